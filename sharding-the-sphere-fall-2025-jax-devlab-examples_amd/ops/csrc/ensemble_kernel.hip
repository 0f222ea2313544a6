// Ensemble statistics of one field of a batched state [M][F][S] (padded layout,
// ops/ensemble_stats.py; the PyTorch twin: models/ensemble_stats.py).
//
//  cells  one thread per interior cell: over the members in ascending order
//           mean = ((x_0 + x_1) + ...) / M
//           var  = (sum_m (x_m - mean)^2) / M        (population variance)
//         in float64 whatever the state's type, stored to mean / var [T][n][n];
//         then the block's record (sum A mean, sum A var, sum A, max var) by a
//         fixed-order tree over the block's 256 threads.
//  fold   one workgroup: lane k < 4 adds (k = 3: maximises) record entry k of
//         every block in ascending block order, so the four scalars are the same
//         numbers on every run.
//
// One workgroup per 16 x 16 cell block of a tile (ragged at the tile end), 256
// threads.  A member's cell is read twice (mean, then deviations); the second
// read hits the vector L1.  Contraction is off in this file: the squared
// deviation is rounded before it is added, as the twin does (d * d, then +).
// Plain C++ and vector loads / stores only; no atomics, nothing persistent.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int EB = 16;          // block edge
constexpr int ENT = EB * EB;    // threads

struct KArgs {
  const void* Q;
  const void* area;
  double* mean;
  double* var;
  double* partials;
  double* out;
  long long member_stride;
  int members, field, ntile, n, S, mg, pw, nb, nblocks;
};

template <typename T>
__global__ __launch_bounds__(ENT) void ens_cells_kernel(const KArgs a) {
  __shared__ double s_r[4][ENT];
  int blk = blockIdx.x;
  const int xb = blk % a.nb;
  blk /= a.nb;
  const int yb = blk % a.nb;
  const int t = blk / a.nb;
  const int tid = threadIdx.x;
  const int x = xb * EB + (tid & (EB - 1)), y = yb * EB + (tid >> 4);
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  if (x < a.n && y < a.n) {
    const size_t c = (size_t)a.field * (size_t)a.S + (size_t)((t * a.pw + y + a.mg) * a.pw + x + a.mg);
    const T* q = (const T*)a.Q + c;
    double s = (double)q[0];
    for (int m = 1; m < a.members; ++m) s = s + (double)q[(size_t)m * (size_t)a.member_stride];
    const double mean = s / (double)a.members;
    double v = 0.0;
    for (int m = 0; m < a.members; ++m) {
      const double d = (double)q[(size_t)m * (size_t)a.member_stride] - mean;
      const double d2 = d * d;
      v = v + d2;
    }
    const double var = v / (double)a.members;
    const size_t cell = ((size_t)t * a.n + y) * a.n + x;
    a.mean[cell] = mean;
    a.var[cell] = var;
    const double A = (double)((const T*)a.area)[cell];
    r0 = A * mean;
    r1 = A * var;
    r2 = A;
    r3 = var;
  }
  s_r[0][tid] = r0;
  s_r[1][tid] = r1;
  s_r[2][tid] = r2;
  s_r[3][tid] = r3;
  __syncthreads();
  for (int h = ENT / 2; h > 0; h >>= 1) {
    if (tid < h) {
      s_r[0][tid] = s_r[0][tid] + s_r[0][tid + h];
      s_r[1][tid] = s_r[1][tid] + s_r[1][tid + h];
      s_r[2][tid] = s_r[2][tid] + s_r[2][tid + h];
      // a NaN variance must reach the maximum: fmax would drop it
      const double p = s_r[3][tid], o = s_r[3][tid + h];
      s_r[3][tid] = (p != p || o != o) ? (p + o) : (p > o ? p : o);
    }
    __syncthreads();
  }
  if (tid < 4) a.partials[(size_t)blockIdx.x * 4 + tid] = s_r[tid][0];
}

__global__ __launch_bounds__(64) void ens_fold_kernel(const double* __restrict__ partials, int nblocks,
                                                      double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= 4) return;
  double acc = partials[k];
  for (int b = 1; b < nblocks; ++b) {
    const double p = partials[(size_t)b * 4 + k];
    if (k < 3) acc = acc + p;
    else acc = (acc != acc || p != p) ? (acc + p) : (acc > p ? acc : p);
  }
  out[k] = acc;
}

template <typename T>
int launch(const EnsStatsDesc* d, hipStream_t s) {
  KArgs a;
  a.Q = d->Q;
  a.area = d->area;
  a.mean = d->mean;
  a.var = d->var;
  a.partials = d->partials;
  a.out = d->out;
  a.member_stride = d->member_stride;
  a.members = d->members;
  a.field = d->field;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nb = (d->n + EB - 1) / EB;
  a.nblocks = d->nblocks;
  hipLaunchKernelGGL((ens_cells_kernel<T>), dim3(d->nblocks), dim3(ENT), 0, s, a);
  if (hipGetLastError() != hipSuccess) return 3;
  hipLaunchKernelGGL(ens_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)d->partials, d->nblocks, d->out);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_ensemble_stats_desc_size(void) { return (int)sizeof(EnsStatsDesc); }

// 1: a descriptor that does not describe a batched state; 2: unknown dtype; 3: launch error
extern "C" int stsp_ensemble_stats_launch(int dtype, const EnsStatsDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || d->mg < 0 || d->members < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  if (d->fields < 1 || d->field < 0 || d->field >= d->fields) return 1;
  if (d->member_stride < (long long)d->fields * d->S) return 1;
  const int nb = (d->n + EB - 1) / EB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->Q || !d->area || !d->mean || !d->var || !d->partials || !d->out) return 1;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
