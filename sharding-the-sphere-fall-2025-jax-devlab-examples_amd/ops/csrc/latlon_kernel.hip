// Longitude-latitude regridding on the device: scalar fields, zonal and
// meridional wind, zonal means.  The definitions are those of models/latlon.py,
// the PyTorch twin; the tables (four source cells and four fp64 weights per
// target point, unit east / north vectors) are built there, on the host.
//
// Two ordinary launches on the caller's stream, nothing persistent, no atomics,
// no polling:
//
//  gather   one thread per target point k = j nlon + i, 256-thread workgroups,
//           ragged tail.  The point's four indices are one 16-byte load and its
//           four weights one 32-byte load; the weights are converted once to the
//           state's type.  A slot of index -1 (a source another rank owns)
//           contributes 0 and reads nothing; the sum is ((t0 + t1) + t2) + t3
//           with t = w x.  Scalar mode loops over C channels of stride `cs`;
//           velocity mode reads h and M at each source, divides (IEEE division)
//           and emits the three Cartesian components.  Stores to partial [C][K]
//           are coalesced along lon.  The source layout (padded state or
//           unpadded tiles) is only a matter of which index table is passed:
//           no integer division here.  Sources are real cells, never ghost
//           slots, so the result does not depend on the ghost ring.
//  finish   one workgroup per latitude row: optional projection of the
//           Cartesian triple onto east / north (out [2][K]), then the zonal mean
//           of every channel: fp64 accumulators whatever the state type, each
//           thread over lon = tid, tid + 256, ... in order, a fixed shuffle
//           tree inside each wave, the four waves folded in wave order through
//           LDS, then divided by nlon.  nlon need not be a multiple of 64 and
//           the result repeats bit for bit.
//
// With several ranks each rank runs the gather on its own cells in `terms` mode:
// it stores the four terms t0 .. t3 of every point and channel ([C][4][K], 0 for
// a slot it does not own) instead of their sum.  The caller adds the ranks'
// arrays in ascending rank order (every term is owned by one rank, so this adds
// zeros: exact) and the finish launch folds ((t0 + t1) + t2) + t3 itself.  The
// result is then the one-rank expression bit for bit, whatever the partition.
//
// Contraction is off in this file: every product and sum rounds on its own, in
// the association the twin writes down, so the one-rank fields differ from the
// twin's only where a division does.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LB = 256;   // workgroup size of both kernels

struct alignas(16) Idx4 {
  int i[4];
};
struct alignas(32) W4 {
  double w[4];
};

template <typename T>
__global__ __launch_bounds__(LB) void latlon_gather_kernel(const T* __restrict__ Q, const Idx4* __restrict__ idx,
                                                           const W4* __restrict__ wt, T* __restrict__ partial,
                                                           int K, int C, size_t cs, int velocity, int terms) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= K) return;
  const Idx4 id = idx[k];
  const W4 wd = wt[k];
  T w[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) w[s] = (T)wd.w[s];
  if (velocity) {
    T t[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      t[s][0] = t[s][1] = t[s][2] = T(0);
      if (id.i[s] >= 0) {
        const size_t c = (size_t)id.i[s];
        const T h = Q[c];
        const T d = h != T(0) ? h : T(1);
        t[s][0] = w[s] * (Q[cs + c] / d);
        t[s][1] = w[s] * (Q[2 * cs + c] / d);
        t[s][2] = w[s] * (Q[3 * cs + c] / d);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (terms) {
#pragma unroll
        for (int s = 0; s < 4; ++s) partial[(size_t)(4 * c + s) * K + k] = t[s][c];
      } else {
        partial[(size_t)c * K + k] = ((t[0][c] + t[1][c]) + t[2][c]) + t[3][c];
      }
    }
    return;
  }
  for (int c = 0; c < C; ++c) {
    const T* q = Q + (size_t)c * cs;
    T t[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = id.i[s] >= 0 ? w[s] * q[id.i[s]] : T(0);
    if (terms) {
#pragma unroll
      for (int s = 0; s < 4; ++s) partial[(size_t)(4 * c + s) * K + k] = t[s];
    } else {
      partial[(size_t)c * K + k] = ((t[0] + t[1]) + t[2]) + t[3];
    }
  }
}

// channel c at point k of the gather's output: the sum itself, or the fold of its four terms
template <typename T>
__device__ __forceinline__ T channel(const T* __restrict__ p, int terms, size_t K, int c, size_t k) {
  if (!terms) return p[(size_t)c * K + k];
  const T* q = p + (size_t)(4 * c) * K + k;
  return ((q[0] + q[K]) + q[2 * K]) + q[3 * K];
}

// sum of one value per thread over the workgroup: shuffle tree per wave, waves in order
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();   // red may still be read from the previous channel
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T>
__global__ __launch_bounds__(LB) void latlon_finish_kernel(const T* __restrict__ partial, const double* __restrict__ east,
                                                           const double* __restrict__ north, T* __restrict__ out,
                                                           double* __restrict__ zm, int K, int nlat, int nlon, int C,
                                                           int project, int terms) {
  __shared__ double red[LB / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const size_t k0 = (size_t)row * nlon;
  const double cnt = (double)nlon;
  if (project) {
    double su = 0.0, sv = 0.0;
    for (int i = tid; i < nlon; i += LB) {
      const size_t k = k0 + i;
      const T x = channel(partial, terms, K, 0, k), y = channel(partial, terms, K, 1, k),
              z = channel(partial, terms, K, 2, k);
      const T u = (x * (T)east[3 * k] + y * (T)east[3 * k + 1]) + z * (T)east[3 * k + 2];
      const T v = (x * (T)north[3 * k] + y * (T)north[3 * k + 1]) + z * (T)north[3 * k + 2];
      out[k] = u;
      out[(size_t)K + k] = v;
      su += (double)u;
      sv += (double)v;
    }
    if (zm) {
      su = block_sum(su, red);
      sv = block_sum(sv, red);
      if (tid == 0) {
        zm[row] = su / cnt;
        zm[(size_t)nlat + row] = sv / cnt;
      }
    }
    return;
  }
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (int i = tid; i < nlon; i += LB) {
      const T x = channel(partial, terms, K, c, k0 + i);
      if (terms) out[(size_t)c * K + k0 + i] = x;
      s += (double)x;
    }
    s = block_sum(s, red);
    if (tid == 0) zm[(size_t)c * nlat + row] = s / cnt;
  }
}

template <typename T>
int launch(const LatLonDesc* d, hipStream_t s) {
  if (d->phases & 1)
    hipLaunchKernelGGL(latlon_gather_kernel<T>, dim3((d->K + LB - 1) / LB), dim3(LB), 0, s, (const T*)d->Q,
                       (const Idx4*)d->idx, (const W4*)d->w, (T*)d->partial, d->K, d->C, (size_t)d->cs, d->velocity,
                       d->terms);
  if (d->phases & 2)
    hipLaunchKernelGGL(latlon_finish_kernel<T>, dim3(d->nlat), dim3(LB), 0, s, (const T*)d->partial, d->east,
                       d->north, (T*)d->out, d->zm, d->K, d->nlat, d->nlon, d->C, d->project, d->terms);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_latlon_desc_size(void) { return (int)sizeof(LatLonDesc); }

extern "C" int stsp_latlon_launch(int dtype, const LatLonDesc* d, hipStream_t stream) {
  if (!d || d->nlat <= 0 || d->nlon <= 0 || d->C <= 0 || d->cs <= 0) return 1;
  if ((long long)d->K != (long long)d->nlat * d->nlon || d->K <= 0) return 1;
  if (!(d->phases & 3) || (d->phases & ~3) || !d->partial) return 1;
  if ((d->phases & 1) && (!d->Q || !d->idx || !d->w)) return 1;
  if (d->velocity && d->C != 3) return 1;
  if (d->phases & 2) {
    if (d->project && (d->C != 3 || !d->east || !d->north)) return 1;
    if ((d->project || d->terms) && !d->out) return 1;
    if (!d->project && !d->zm) return 1;
  }
  if (((uintptr_t)d->idx & 15) || ((uintptr_t)d->w & 31)) return 1;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
