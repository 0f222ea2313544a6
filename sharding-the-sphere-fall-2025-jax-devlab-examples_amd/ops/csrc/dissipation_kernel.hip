// Scale-selective dissipation of the shallow-water state on the device: the
// consistent Laplacian of models/dissipation.py (the PyTorch twin) in two passes.
//
//  pass 1  one thread per cell: its four scalars w = (h, M / h) (or the four rows
//          of a float64 buffer as they are) and those of its four face
//          neighbours, the least-squares gradient G = sum_k W_k (w_k - w_i) of each
//          scalar; 16 float64 rows to the scratch [16][S], padded layout.
//  pass 2  one thread per cell: for each of its four edges the neighbour's 16
//          scratch rows, the corrected flux  c (s_R - s_L) + 1/2 (G_L + G_R) . k,
//          then L w = (dPhi_x + dPhi_y) / A; L w is stored, or the state is
//          updated in place: h' = h + coef L_0, v' = P (v + coef L_1..3), M' = h' v'.
//
// A neighbour inside the tile is the adjacent cell of the padded layout; one
// across a tile side comes through gmap (>= 0: the source cell's padded offset on
// this rank, an interior cell; < 0: a row of the receive buffer), never from a
// ghost slot.  Pass 2 reads the scratch (and, for the update, the thread's own
// state cell) only, so the state it writes is never a neighbour's input.
//
// One workgroup per 16 x 16 cell block of a tile (ragged at the tile end), 256
// threads, no LDS and no barrier: both passes are bound by their table and
// scratch traffic (pass 1 reads 12 weight planes and writes 16 rows per cell,
// pass 2 reads 16 rows and 8 edge-table planes), a cell's rows are reused by four
// neighbours only and those reads hit the vector L1 or the L2.  A block row is 16
// consecutive doubles, one 128-byte line per plane, and every table is stored
// one plane per component, so a half-row of lanes reads each plane with unit
// stride.
//
// All arithmetic is float64 whatever the state's type: an fp32 state is converted
// at load and rounded once at store.  Contraction is off in this file: every
// product and sum rounds on its own, in the association the twin writes down.
// Plain C++ and vector stores only; no atomics, nothing persistent.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int DB = 16;          // block edge
constexpr int ROWS = 16;        // scratch rows

struct KArgs {
  const void* src;
  const void* recv;
  double* scratch;
  const double* srecv;
  void* out;
  const int* gmap;
  const double* W;
  const double* cx;
  const double* cy;
  const double* kx;
  const double* ky;
  const double* gb;
  const double* dbx;
  const double* dby;
  const double* invA;
  const double* ctr;
  int ntile, n, S, mg, pw, nbx, nby, recv_stride, use_b, depth;
  double coef;
};

// (tile, x, y) of this thread's cell; false: outside the ragged block
__device__ __forceinline__ bool decode(const KArgs& a, int& t, int& x, int& y) {
  int blk = blockIdx.x;
  const int xb = blk % a.nbx;
  blk /= a.nbx;
  const int yb = blk % a.nby;
  t = blk / a.nby;
  x = xb * DB + (threadIdx.x & (DB - 1));
  y = yb * DB + (threadIdx.x >> 4);
  return x < a.n && y < a.n;
}

// ghost-map codes of the neighbours W, E, S, N of interior cell (x, y), padded offset c
__device__ __forceinline__ void neighbours(const KArgs& a, int t, int x, int y, int c, int code[4]) {
  const int n = a.n;
  const int* g = a.gmap + (size_t)t * 4 * a.mg * n;
  const size_t side = (size_t)a.mg * n;
  code[0] = x > 0 ? c - 1 : g[y];
  code[1] = x < n - 1 ? c + 1 : g[side + y];
  code[2] = y > 0 ? c - a.pw : g[2 * side + x];
  code[3] = y < n - 1 ? c + a.pw : g[3 * side + x];
}

// the four scalars behind code c of the pass-1 input: SWE (h, M / h), else the rows as stored
template <typename T, bool SWE>
__device__ __forceinline__ void load_w(const KArgs& a, int c, double w[4]) {
  if (c >= 0) {
    const T* q = (const T*)a.src + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (double)q[(size_t)k * a.S];
  } else {
    const T* r = (const T*)a.recv + (size_t)a.recv_stride * (size_t)(-1 - c);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (double)r[k];
  }
  if (SWE) {
    const double s = w[0] != 0.0 ? w[0] : 1.0;
    w[1] = w[1] / s;
    w[2] = w[2] / s;
    w[3] = w[3] / s;
  }
}

template <typename T, bool SWE>
__global__ __launch_bounds__(256) void dissipation_gradient_kernel(const KArgs a) {
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int n = a.n;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  int code[4];
  neighbours(a, t, x, y, c, code);
  double w0[4], d[4][4];          // d[k][s]: neighbour k minus own, scalar s
  load_w<T, SWE>(a, c, w0);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double wk[4];
    load_w<T, SWE>(a, code[k], wk);
#pragma unroll
    for (int s = 0; s < 4; ++s) d[k][s] = wk[s] - w0[s];
  }
  const size_t cells = (size_t)a.ntile * n * n;
  const size_t cell = ((size_t)t * n + y) * n + x;
  double* sc = a.scratch + c;
#pragma unroll
  for (int s = 0; s < 4; ++s) sc[(size_t)s * a.S] = w0[s];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double wW = a.W[(size_t)(0 * 3 + j) * cells + cell], wE = a.W[(size_t)(1 * 3 + j) * cells + cell];
    const double wS = a.W[(size_t)(2 * 3 + j) * cells + cell], wN = a.W[(size_t)(3 * 3 + j) * cells + cell];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      double g = ((wW * d[0][s] + wE * d[1][s]) + wS * d[2][s]) + wN * d[3][s];
      if (s == 0 && a.use_b) g = g + a.gb[(size_t)j * cells + cell];
      sc[(size_t)(4 + 3 * s + j) * a.S] = g;
    }
  }
}

// the 16 scratch rows behind code c
__device__ __forceinline__ void load_rows(const KArgs& a, int c, double r[ROWS]) {
  if (c >= 0) {
    const double* q = a.scratch + c;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) r[k] = q[(size_t)k * a.S];
  } else {
    const double* q = a.srecv + (size_t)ROWS * (size_t)(-1 - c);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) r[k] = q[k];
  }
}

// fluxes of the four scalars through one edge: left rows l, right rows r, c_e, k_e, b_R - b_L
__device__ __forceinline__ void edge_flux(const double l[ROWS], const double r[ROWS], double ce, const double k[3],
                                          double db, double phi[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    double ds = r[s] - l[s];
    if (s == 0) ds = ds + db;     // db = 0 where the topography terms are off
    const double g0 = l[4 + 3 * s] + r[4 + 3 * s], g1 = l[5 + 3 * s] + r[5 + 3 * s], g2 = l[6 + 3 * s] + r[6 + 3 * s];
    phi[s] = ce * ds + 0.5 * ((g0 * k[0] + g1 * k[1]) + g2 * k[2]);
  }
}

template <typename T, bool UPDATE>
__global__ __launch_bounds__(256) void dissipation_flux_kernel(const KArgs a) {
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int n = a.n;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  int code[4];
  neighbours(a, t, x, y, c, code);
  double own[ROWS], nb[ROWS], pW[4], pE[4], pS[4], pN[4], k[3];
  load_rows(a, c, own);
  const size_t n1 = n + 1;
  // x-edge tables [T][n][n+1] (vectors: one plane per component), y-edge tables [T][n+1][n]
  const size_t ex = ((size_t)t * n + y) * n1 + x, px = (size_t)a.ntile * n * n1;
  const size_t ey = ((size_t)t * n1 + y) * n + x, py = (size_t)a.ntile * n1 * n;
  const bool ub = a.use_b != 0;
  load_rows(a, code[0], nb);
  k[0] = a.kx[ex], k[1] = a.kx[px + ex], k[2] = a.kx[2 * px + ex];
  edge_flux(nb, own, a.cx[ex], k, ub ? a.dbx[ex] : 0.0, pW);
  load_rows(a, code[1], nb);
  k[0] = a.kx[ex + 1], k[1] = a.kx[px + ex + 1], k[2] = a.kx[2 * px + ex + 1];
  edge_flux(own, nb, a.cx[ex + 1], k, ub ? a.dbx[ex + 1] : 0.0, pE);
  load_rows(a, code[2], nb);
  k[0] = a.ky[ey], k[1] = a.ky[py + ey], k[2] = a.ky[2 * py + ey];
  edge_flux(nb, own, a.cy[ey], k, ub ? a.dby[ey] : 0.0, pS);
  load_rows(a, code[3], nb);
  k[0] = a.ky[ey + n], k[1] = a.ky[py + ey + n], k[2] = a.ky[2 * py + ey + n];
  edge_flux(own, nb, a.cy[ey + n], k, ub ? a.dby[ey + n] : 0.0, pN);
  const size_t cells = (size_t)a.ntile * n * n;
  const size_t cell = ((size_t)t * n + y) * n + x;
  const double invA = a.invA[cell];
  double L[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) L[s] = ((pE[s] - pW[s]) + (pN[s] - pS[s])) * invA;
  if (!UPDATE) {
    double* o = (double*)a.out + c;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[(size_t)s * a.S] = L[s];
    return;
  }
  // update of the thread's own state cell, in place
  T* q = (T*)a.out + c;
  const double h0 = (double)q[0];
  const double sf = h0 != 0.0 ? h0 : 1.0;
  const double h = a.depth ? h0 + a.coef * L[0] : h0;
  double u[3], r[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    u[j] = (double)q[(size_t)(j + 1) * a.S] / sf + a.coef * L[j + 1];
    r[j] = a.ctr[(size_t)j * cells + cell];
  }
  const double dd = (u[0] * r[0] + u[1] * r[1]) + u[2] * r[2];
  if (a.depth) q[0] = (T)h;
#pragma unroll
  for (int j = 0; j < 3; ++j) q[(size_t)(j + 1) * a.S] = (T)(h * (u[j] - dd * r[j]));
}

template <typename T>
int launch(const DissDesc* d, hipStream_t s) {
  KArgs a;
  a.src = d->src;
  a.recv = d->recv;
  a.scratch = d->scratch;
  a.srecv = d->srecv;
  a.out = d->out;
  a.gmap = d->gmap;
  a.W = d->W;
  a.cx = d->cx;
  a.cy = d->cy;
  a.kx = d->kx;
  a.ky = d->ky;
  a.gb = d->gb;
  a.dbx = d->dbx;
  a.dby = d->dby;
  a.invA = d->invA;
  a.ctr = d->ctr;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nbx = a.nby = (d->n + DB - 1) / DB;
  a.recv_stride = d->recv_stride;
  a.use_b = d->use_b;
  a.depth = d->depth;
  a.coef = d->coef;
  const dim3 grid(d->nblocks), block(256);
  if (d->pass_ == 1) {
    // mode 0 reads float64 rows whatever the state's type
    if (d->mode)
      hipLaunchKernelGGL((dissipation_gradient_kernel<T, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((dissipation_gradient_kernel<double, false>), grid, block, 0, s, a);
  } else {
    if (d->mode)
      hipLaunchKernelGGL((dissipation_flux_kernel<T, true>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((dissipation_flux_kernel<double, false>), grid, block, 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_dissipation_desc_size(void) { return (int)sizeof(DissDesc); }

extern "C" int stsp_dissipation_launch(int dtype, const DissDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || d->mg < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  const int nb = (d->n + DB - 1) / DB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->scratch || !d->gmap || !d->W || !d->cx || !d->cy || !d->kx || !d->ky || !d->gb || !d->dbx || !d->dby ||
      !d->invA || !d->ctr)
    return 1;
  if (d->nrecv < 0) return 1;
  if (d->pass_ == 1) {
    if (!d->src || (d->nrecv > 0 && (!d->recv || d->recv_stride < 4))) return 1;
  } else if (d->pass_ == 2) {
    if (!d->out || (d->nrecv > 0 && !d->srecv)) return 1;
  } else {
    return 1;
  }
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
