// Snapshot EOFs (method of snapshots) of S <= 64 snapshots over the cells
// (ops/eof.py; definitions and the PyTorch twin: models/eof.py).  Everything is
// float64; float32 snapshots are converted at load.
//
// The snapshots are either contiguous [S][cells] or one field of the batched
// padded state [M][F][S_pad] (snapshot = member): launch values of the same
// kernels.  A cell's flat index g (tile-major [T][n][n] in the padded mode) is
// turned into its storage offset by cell_offset(); ghost slots have no flat
// index and are never addressed.
//
//  gram   one workgroup (4 waves) per slab of cell tiles, a tile being 64 cells.
//         Per tile: wave w loads the rows s = w, w + 4, .. of the tile (one
//         coalesced row of 64 cells per load) into registers one tile ahead, the
//         raw values go to the LDS tile Z [Spad][64 + 2], and wave w forms the
//         mean of its 16 cells (ascending s) and sqrt(a).  Wave w then owns the
//         k-steps of its 16 cells: per step one operand per 16-row block,
//         z = (Z - mean) sqrt(a) (0 in the rows beyond S), serves as A and B of
//         v_mfma_f64_16x16x4 for the upper-triangle tiles of Z Z^T, which stay in
//         registers across the slab.  The row stride 66 makes the operand reads
//         (16 rows x 2 cells per half wave) hit 32 distinct 8-byte banks.  At the
//         end the four waves' accumulators are added in wave order through LDS
//         and the slab's partial [Spad][Spad] (upper tiles) is stored.
//  fold   one thread per entry of the upper tiles: the partials in ascending
//         slab order, divided by S - 1, stored with its mirror image.  No atomics:
//         C does not depend on which CU ran which slab.
//  eigen  one workgroup: cyclic two-sided Jacobi on the leading Me x Me part
//         (Me = S rounded up to even), A and V in dynamic LDS with row stride
//         Me + 1 (67,864 bytes at S = 64: above 64 KiB, so the launch raises the
//         kernel's dynamic-LDS limit first).  Round-robin pairs, the disjoint
//         rotations of a step applied by all threads (rows, then columns of A and
//         V).  A pair is rotated while |a_pq| > 1e-15 sqrt(a_pp a_qq), as in
//         letkf_kernel.hip; C is only semi-definite here (the anomalies sum to
//         zero), so entries below 1e-22 trace(C) are left as well.  The first
//         sweep that rotates nothing ends it; the sweep cap sets err[0].  Then
//         the descending order (rank sort), the sign convention, the zero-mode
//         rule, U^T [Kpad][Spad] = v_k / sqrt((S-1) lam_k) and the principal
//         components.
//  proj   the slab and tile walk of gram without sqrt(a).  Wave w < Kpad / 16
//         holds its 16 rows of U^T in registers (A operand) and multiplies them
//         by the four 16-cell blocks of the tile (B operand from LDS); the
//         pattern rows are stored, and the mean from the same pass.
//
// The snapshots are read twice in all.  Nothing uses scratch; plain C++ and
// vector loads / stores only.
#include "stsp_kernels.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int TC = 64;            // cells of a tile
constexpr int LDZ = TC + 2;       // row stride of the LDS tile
constexpr int NTH = 256;          // threads (4 waves)
constexpr int SWEEP_CAP = 40;
constexpr double ROT_EPS = 1e-15;     // relative size of an off-diagonal entry that is still rotated
constexpr double ROT_FLOOR = 1e-22;   // .. and its size relative to trace(C)
constexpr double F64_EPS = 2.220446049250313e-16;

struct KArgs {
  const void* X;
  const double* w;
  const double* U;
  double* partials;
  double* patterns;
  double* mean;
  long long snap_stride, origin;
  int S, k, cells, rowlen, tile_rows, row_pitch, tile_pitch, slab_tiles, ntiles;
};

// storage offset of the cell with flat index g < cells
__device__ __forceinline__ size_t cell_offset(const KArgs& a, int g) {
  const int row = g / a.rowlen, x = g - row * a.rowlen;
  const int t = row / a.tile_rows, y = row - t * a.tile_rows;
  return (size_t)a.origin + (size_t)t * (size_t)a.tile_pitch + (size_t)y * (size_t)a.row_pitch + (size_t)x;
}

// rows s = wv, wv + 4, .. of cell tile `tile` at cell `lane`: zeros beyond S and beyond the cells
template <typename T, int RPW>
__device__ __forceinline__ void load_rows(const KArgs& a, int tile, int wv, int lane, double (&pre)[RPW]) {
  const int g = tile * TC + lane;
  const bool in = g < a.cells;
  const T* p = (const T*)a.X + (in ? cell_offset(a, g) : (size_t)0);
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int s = wv + 4 * i;
    pre[i] = (in && s < a.S) ? (double)p[(size_t)s * (size_t)a.snap_stride] : 0.0;
  }
}

// the raw tile into LDS, the next one into registers, the mean (and the weight's root) of the
// wave's 16 cells; ends behind a workgroup barrier
template <typename T, int RPW>
__device__ __forceinline__ void stage_tile(const KArgs& a, int tile, int tile1, int wv, int lane, double (&pre)[RPW],
                                           double* s_z, double* s_mean, double* s_sq) {
#pragma unroll
  for (int i = 0; i < RPW; ++i) s_z[(wv + 4 * i) * LDZ + lane] = pre[i];
  __syncthreads();
  if (tile + 1 < tile1) load_rows<T, RPW>(a, tile + 1, wv, lane, pre);
  const int c = wv * 16 + (lane & 15);
  double sum = s_z[c];
  for (int s = 1; s < a.S; ++s) sum = sum + s_z[s * LDZ + c];
  if (lane < 16) {
    const int g = tile * TC + c;
    s_mean[c] = sum / (double)a.S;
    if (s_sq) s_sq[c] = g < a.cells ? sqrt(a.w[g]) : 0.0;
  }
  __syncthreads();
}

template <typename T, int NT>
__global__ __launch_bounds__(NTH) void eof_gram_kernel(const KArgs a) {
  constexpr int SP = 16 * NT, RPW = 4 * NT, NTRI = NT * (NT + 1) / 2;
  __shared__ double s_z[SP * LDZ > NTRI * 256 ? SP * LDZ : NTRI * 256];
  __shared__ double s_mean[TC];
  __shared__ double s_sq[TC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i16 = lane & 15, q = lane >> 4;
  const int tile0 = blockIdx.x * a.slab_tiles;
  const int tile1 = tile0 + a.slab_tiles < a.ntiles ? tile0 + a.slab_tiles : a.ntiles;
  d4 acc[NTRI];
#pragma unroll
  for (int i = 0; i < NTRI; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  double pre[RPW];
  load_rows<T, RPW>(a, tile0, wv, lane, pre);
  for (int tile = tile0; tile < tile1; ++tile) {
    stage_tile<T, RPW>(a, tile, tile1, wv, lane, pre, s_z, s_mean, s_sq);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int cc = wv * 16 + ks * 4 + q;
      const double m = s_mean[cc], sq = s_sq[cc];
      double z[NT];
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const int row = b * 16 + i16;
        z[b] = row < a.S ? (s_z[row * LDZ + cc] - m) * sq : 0.0;
      }
      int idx = 0;
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = i; j < NT; ++j, ++idx) acc[idx] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[i], z[j], acc[idx], 0, 0, 0);
    }
    __syncthreads();
  }
  // ---- ((wave 0 + wave 1) + wave 2) + wave 3, every lane on its own slots ----------------
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
      int idx = 0;
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = i; j < NT; ++j, ++idx)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* slot = s_z + (idx * 4 + r) * 64 + lane;
            const double v = w == 0 ? acc[idx][r] : *slot + acc[idx][r];
            if (w < 3) *slot = v;
            else a.partials[(size_t)blockIdx.x * (SP * SP) + (size_t)(16 * i + 4 * r + q) * SP + 16 * j + i16] = v;
          }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(NTH) void eof_fold_kernel(const double* __restrict__ partials, int slabs, int SP, int S,
                                                       double* __restrict__ C) {
  const int e = blockIdx.x * NTH + threadIdx.x;
  if (e >= SP * SP) return;
  const int row = e / SP, col = e - row * SP;
  if (row > col) return;            // the upper triangle; the mirror image is stored with it
  double acc = 0.0;
  for (int b = 0; b < slabs; ++b) acc = acc + partials[(size_t)b * (size_t)(SP * SP) + e];
  const double v = (row < S && col < S) ? acc / (double)(S - 1) : 0.0;
  C[row * SP + col] = v;
  C[col * SP + row] = v;
}

struct EArgs {
  const double* C;
  double* U;
  double* values;
  double* total;
  double* pcs;
  int* err;
  int S, SP, k, KP;
};

__global__ __launch_bounds__(NTH) void eof_eigen_kernel(const EArgs a) {
  extern __shared__ __align__(16) unsigned char eof_smem[];
  const int S = a.S, Me = (S + 1) & ~1, LD = Me + 1, np = Me / 2, tid = threadIdx.x;
  double* A = reinterpret_cast<double*>(eof_smem);
  double* V = A + Me * LD;
  double* s_cs = V + Me * LD;         // (c, s) of the step's pairs; then the modes' signs
  double* s_lam = s_cs + 64;          // eigenvalues
  double* s_tot = s_lam + 64;         // [2] trace(C)
  int* s_pq = reinterpret_cast<int*>(s_tot + 2);   // (p, q) of the step's pairs; then the order
  int* s_flag = s_pq + 64;

  for (int e = tid; e < Me * Me; e += NTH) {
    const int i = e / Me, j = e - i * Me;
    A[i * LD + j] = (i < S && j < S) ? a.C[i * a.SP + j] : 0.0;
    V[i * LD + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < S; ++i) t = t + A[i * LD + i];
    s_tot[0] = t;
  }
  __syncthreads();
  const double total = s_tot[0], floor_abs = ROT_FLOOR * total;

  for (int sw = 0;; ++sw) {
    if (sw >= SWEEP_CAP) {
      if (tid == 0) a.err[0] = 1;
      break;
    }
    if (tid == 0) s_flag[0] = 0;
    __syncthreads();
    for (int st = 0; st < Me - 1; ++st) {
      if (tid < np) {
        int p, q;
        if (tid == 0) {
          p = Me - 1;
          q = st;
        } else {
          p = (st + tid) % (Me - 1);
          q = (st - tid + Me - 1) % (Me - 1);
        }
        if (p > q) {
          const int sp = p;
          p = q;
          q = sp;
        }
        const double apq = A[p * LD + q], app = A[p * LD + p], aqq = A[q * LD + q];
        const double pr = app * aqq;
        const double rel = pr > 0.0 ? ROT_EPS * sqrt(pr) : 0.0;
        double c = 1.0, s = 0.0;
        if (fabs(apq) > (rel > floor_abs ? rel : floor_abs)) {
          const double tau = (aqq - app) / (2.0 * apq);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + tt * tt);
          s = tt * c;
          s_flag[0] = 1;
        }
        s_cs[2 * tid] = c;
        s_cs[2 * tid + 1] = s;
        s_pq[2 * tid] = p;
        s_pq[2 * tid + 1] = q;
      }
      __syncthreads();
      for (int e = tid; e < np * Me; e += NTH) {          // rows: A <- J^T A
        const int pi = e / Me, j = e - pi * Me;
        const int p = s_pq[2 * pi], q = s_pq[2 * pi + 1];
        const double c = s_cs[2 * pi], s = s_cs[2 * pi + 1];
        const double ap = A[p * LD + j], aq = A[q * LD + j];
        A[p * LD + j] = c * ap - s * aq;
        A[q * LD + j] = s * ap + c * aq;
      }
      __syncthreads();
      for (int e = tid; e < np * Me; e += NTH) {          // columns: A <- A J, V <- V J
        const int pi = e / Me, i = e - pi * Me;
        const int p = s_pq[2 * pi], q = s_pq[2 * pi + 1];
        const double c = s_cs[2 * pi], s = s_cs[2 * pi + 1];
        const double ap = A[i * LD + p], aq = A[i * LD + q];
        A[i * LD + p] = c * ap - s * aq;
        A[i * LD + q] = s * ap + c * aq;
        const double vp = V[i * LD + p], vq = V[i * LD + q];
        V[i * LD + p] = c * vp - s * vq;
        V[i * LD + q] = s * vp + c * vq;
      }
      __syncthreads();
      if (tid < np && s_cs[2 * tid + 1] != 0.0) {         // the annihilated pair is exactly zero
        const int p = s_pq[2 * tid], q = s_pq[2 * tid + 1];
        A[p * LD + q] = 0.0;
        A[q * LD + p] = 0.0;
      }
      __syncthreads();
    }
    const int rotated = s_flag[0];
    __syncthreads();
    if (!rotated) break;
  }

  // ---- descending order (the padding index of an odd S goes last), signs, scales ----------
  if (tid < Me) s_lam[tid] = A[tid * LD + tid];
  __syncthreads();
  if (tid < Me) {
    int rank = 0;
    for (int j = 0; j < Me; ++j) {
      if (j == tid) continue;
      bool before;
      if (tid >= S) before = j < S || j < tid;
      else if (j >= S) before = false;
      else before = s_lam[j] > s_lam[tid] || (s_lam[j] == s_lam[tid] && j < tid);
      rank += before ? 1 : 0;
    }
    s_pq[rank] = tid;
  }
  __syncthreads();
  if (tid < a.KP) {
    double sg = 0.0;
    if (tid < a.k) {
      const int col = s_pq[tid];
      const double lam = s_lam[col];
      double best = -1.0;
      sg = 1.0;
      for (int s = 0; s < S; ++s) {
        const double v = V[s * LD + col];
        if (fabs(v) > best) {
          best = fabs(v);
          sg = v < 0.0 ? -1.0 : 1.0;
        }
      }
      a.values[tid] = lam;
      if (!(lam > (double)S * F64_EPS * total)) sg = 0.0;     // the zero-mode rule
    }
    s_cs[tid] = sg;
  }
  if (tid == 0) a.total[0] = total;
  __syncthreads();
  for (int e = tid; e < a.KP * a.SP; e += NTH) {
    const int m = e / a.SP, s = e - m * a.SP;
    double u = 0.0;
    if (m < a.k && s < S && s_cs[m] != 0.0) {
      const int col = s_pq[m];
      const double sc = sqrt((double)(S - 1) * s_lam[col]);
      const double v = s_cs[m] * V[s * LD + col];
      u = v / sc;
      a.pcs[m * S + s] = sc * v;
    } else if (m < a.k && s < S) {
      a.pcs[m * S + s] = 0.0;
    }
    a.U[e] = u;
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(NTH) void eof_proj_kernel(const KArgs a, int KT) {
  constexpr int SP = 16 * NT, RPW = 4 * NT;
  __shared__ double s_z[SP * LDZ];
  __shared__ double s_mean[TC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i16 = lane & 15, q = lane >> 4;
  const int tile0 = blockIdx.x * a.slab_tiles;
  const int tile1 = tile0 + a.slab_tiles < a.ntiles ? tile0 + a.slab_tiles : a.ntiles;
  // the wave's rows of U^T: mode 16 wv + i16, snapshots 4 ks + q
  double u[RPW];
#pragma unroll
  for (int ks = 0; ks < RPW; ++ks) u[ks] = wv < KT ? a.U[(size_t)(wv * 16 + i16) * SP + 4 * ks + q] : 0.0;
  double pre[RPW];
  load_rows<T, RPW>(a, tile0, wv, lane, pre);
  for (int tile = tile0; tile < tile1; ++tile) {
    stage_tile<T, RPW>(a, tile, tile1, wv, lane, pre, s_z, s_mean, nullptr);
    if (lane < 16) {
      const int g = tile * TC + wv * 16 + lane;
      if (g < a.cells) a.mean[g] = s_mean[wv * 16 + lane];
    }
    if (wv < KT) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int cc = cb * 16 + i16;
        const double m = s_mean[cc];
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < RPW; ++ks) {
          const int s = 4 * ks + q;
          const double b = s < a.S ? s_z[s * LDZ + cc] - m : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(u[ks], b, acc, 0, 0, 0);
        }
        const int g = tile * TC + cc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int mode = wv * 16 + 4 * r + q;
          if (mode < a.k && g < a.cells) a.patterns[(size_t)mode * (size_t)a.cells + g] = acc[r];
        }
      }
    }
    __syncthreads();
  }
}

template <typename T, int NT>
int launch_nt(const EofDesc* d, const KArgs& a, hipStream_t s) {
  const int SP = d->Spad;
  hipLaunchKernelGGL((eof_gram_kernel<T, NT>), dim3(d->slabs), dim3(NTH), 0, s, a);
  if (hipGetLastError() != hipSuccess) return 3;
  hipLaunchKernelGGL(eof_fold_kernel, dim3((SP * SP + NTH - 1) / NTH), dim3(NTH), 0, s, (const double*)d->partials,
                     d->slabs, SP, d->S, d->C);
  if (hipGetLastError() != hipSuccess) return 3;
  EArgs e;
  e.C = d->C;
  e.U = d->U;
  e.values = d->values;
  e.total = d->total;
  e.pcs = d->pcs;
  e.err = d->err;
  e.S = d->S;
  e.SP = SP;
  e.k = d->k;
  e.KP = d->Kpad;
  const size_t lds = (size_t)stsp_eof_eigen_lds(d->S);
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(eof_eigen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return 3;
  }
  hipLaunchKernelGGL(eof_eigen_kernel, dim3(1), dim3(NTH), lds, s, e);
  if (hipGetLastError() != hipSuccess) return 3;
  hipLaunchKernelGGL((eof_proj_kernel<T, NT>), dim3(d->slabs), dim3(NTH), 0, s, a, d->Kpad / 16);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

template <typename T>
int launch(const EofDesc* d, hipStream_t s) {
  KArgs a;
  a.X = d->X;
  a.w = d->w;
  a.U = d->U;
  a.partials = d->partials;
  a.patterns = d->patterns;
  a.mean = d->mean;
  a.snap_stride = d->snap_stride;
  a.S = d->S;
  a.k = d->k;
  a.cells = d->cells;
  if (d->padded) {
    a.origin = (long long)d->field * d->Sp + (long long)d->mg * d->pw + d->mg;
    a.rowlen = d->n;
    a.tile_rows = d->n;
    a.row_pitch = d->pw;
    a.tile_pitch = d->pw * d->pw;
  } else {
    a.origin = 0;
    a.rowlen = d->cells;
    a.tile_rows = 1;
    a.row_pitch = 0;
    a.tile_pitch = 0;
  }
  a.slab_tiles = d->slab_tiles;
  a.ntiles = (d->cells + TC - 1) / TC;
  switch (d->Spad) {
    case 16: return launch_nt<T, 1>(d, a, s);
    case 32: return launch_nt<T, 2>(d, a, s);
    case 48: return launch_nt<T, 3>(d, a, s);
    default: return launch_nt<T, 4>(d, a, s);
  }
}

}  // namespace

extern "C" int stsp_eof_desc_size(void) { return (int)sizeof(EofDesc); }

// dynamic LDS bytes of the eigen phase for S snapshots
extern "C" int stsp_eof_eigen_lds(int S) {
  const int Me = (S + 1) & ~1;
  return (2 * Me * (Me + 1) + 64 + 64 + 2) * 8 + (64 + 2) * 4;
}

// 1: a descriptor that does not describe the snapshots; 2: unknown dtype; 3: launch error;
// 4: snapshots outside 2 .. 64 (or Spad not their tile padding); 5: k outside 1 .. S-1 (or Kpad
// not its tile padding)
extern "C" int stsp_eof_launch(int dtype, const EofDesc* d, hipStream_t stream) {
  if (!d) return 1;
  if (d->S < 2 || d->S > STSP_EOF_MAX_S || d->Spad != 16 * ((d->S + 15) / 16)) return 4;
  if (d->k < 1 || d->k > d->S - 1 || d->Kpad != 16 * ((d->k + 15) / 16)) return 5;
  if (d->cells < 1) return 1;
  if (d->padded) {
    if (d->ntile <= 0 || d->n <= 0 || d->mg < 0 || d->fields < 1 || d->field < 0 || d->field >= d->fields) return 1;
    if (d->pw != d->n + 2 * d->mg || (long long)d->Sp != (long long)d->ntile * d->pw * d->pw) return 1;
    if ((long long)d->cells != (long long)d->ntile * d->n * d->n) return 1;
    if (d->snap_stride < (long long)d->fields * d->Sp) return 1;
  } else if (d->snap_stride < (long long)d->cells) {
    return 1;
  }
  const int ntiles = (d->cells + TC - 1) / TC;
  if (d->slab_tiles < 1 || (long long)d->slabs != ((long long)ntiles + d->slab_tiles - 1) / d->slab_tiles) return 1;
  if (!d->X || !d->w || !d->partials || !d->C || !d->U || !d->values || !d->total || !d->pcs || !d->patterns ||
      !d->mean || !d->err)
    return 1;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
