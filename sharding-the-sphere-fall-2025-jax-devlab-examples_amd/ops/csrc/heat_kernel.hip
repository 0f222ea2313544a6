// Consistent thermal diffusion on the device: dT/dt = kappa L T with the
// consistent Laplacian of models/dissipation.py for one scalar, in two passes per
// Runge-Kutta stage (the PyTorch twin: models/diffusion.py).
//
//  pass 1  one thread per cell: the stage input Q at the cell and at its four face
//          neighbours, the least-squares gradient G = sum_k W_k (Q_k - Q_i); four
//          float64 rows (T, Gx, Gy, Gz) to the scratch [4][S], padded layout.
//  pass 2  one thread per cell: for each of its four edges the neighbour's four
//          scratch rows, the corrected flux  c (T_R - T_L) + 1/2 (G_L + G_R) . k,
//          then L = (dPhi_x + dPhi_y) / A, and one of
//            mode 0   lout = L                                       (float64)
//            mode 1   out  = a2dt kappa L (+ a1 Q) (+ a0 X)
//            mode 2   that, and acc_out = c1 X + c2dt kappa L (+ c0 ACC)
//          in the order of operations of TorchCompute.stage.
//
// A neighbour inside the tile is the adjacent cell of the padded layout; one
// across a tile side comes through gmap (>= 0: the source cell's padded offset on
// this rank, an interior cell; < 0: a row of the receive buffer), never from a
// ghost slot and never from a corner ghost.  The scratch rows of a global
// Cartesian G are exchanged between the passes, which is what makes the operator
// independent of the decomposition: a ring cell's gradient needs that cell's own
// neighbours, at a tile corner the diagonal tile's cells, at a cube corner cells
// of a third panel, so one LDS-tiled launch could not form it.
//
// Pass 2 reads X, Q and ACC at the thread's own cell only, and neighbours only
// from the scratch.  So out may alias X (the last stage of SSP-RK3) or Q, and
// acc_out may alias acc_in (RK4), with no hazard: no thread reads a cell of those
// buffers that another thread writes.
//
// One workgroup per 16 x 16 cell block of a tile (ragged at the tile end), 256
// threads, no LDS and no barrier: both passes are bound by their table and
// scratch traffic, a cell's rows are reused by four neighbours only and those
// reads hit the vector L1 or the L2.  A block row is 16 consecutive doubles, one
// 128-byte line per plane, and every table is stored one plane per component.
//
// All arithmetic is float64 whatever the state's type: an fp32 state is converted
// at load and rounded once at store.  Contraction is off in this file: every
// product and sum rounds on its own, in the association the twin writes down.
// Plain C++ and vector stores only; no atomics, nothing persistent.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int HB = 16;          // block edge
constexpr int ROWS = 4;         // scratch rows

struct KArgs {
  const void* q;
  const void* recv;
  double* scratch;
  const double* srecv;
  const int* gmap;
  const double* W;
  const double* cx;
  const double* cy;
  const double* kx;
  const double* ky;
  const double* invA;
  const void* x;
  const void* acc_in;
  void* out;
  void* acc_out;
  double* lout;
  int ntile, n, S, mg, pw, nbx, nby, recv_stride;
  double kappa, a0, a1, a2dt, c0, c1, c2dt;
};

// (tile, x, y) of this thread's cell; false: outside the ragged block
__device__ __forceinline__ bool decode(const KArgs& a, int& t, int& x, int& y) {
  int blk = blockIdx.x;
  const int xb = blk % a.nbx;
  blk /= a.nbx;
  const int yb = blk % a.nby;
  t = blk / a.nby;
  x = xb * HB + (threadIdx.x & (HB - 1));
  y = yb * HB + (threadIdx.x >> 4);
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

// the stage input behind code c
template <typename T>
__device__ __forceinline__ double load_q(const KArgs& a, int c) {
  if (c >= 0) return (double)((const T*)a.q)[c];
  return (double)((const T*)a.recv)[(size_t)a.recv_stride * (size_t)(-1 - c)];
}

template <typename T>
__global__ __launch_bounds__(256) void heat_gradient_kernel(const KArgs a) {
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int n = a.n;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  int code[4];
  neighbours(a, t, x, y, c, code);
  const double t0 = load_q<T>(a, c);
  double d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = load_q<T>(a, code[k]) - t0;
  const size_t cells = (size_t)a.ntile * n * n;
  const size_t cell = ((size_t)t * n + y) * n + x;
  double* sc = a.scratch + c;
  sc[0] = t0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double wW = a.W[(size_t)(0 * 3 + j) * cells + cell], wE = a.W[(size_t)(1 * 3 + j) * cells + cell];
    const double wS = a.W[(size_t)(2 * 3 + j) * cells + cell], wN = a.W[(size_t)(3 * 3 + j) * cells + cell];
    sc[(size_t)(1 + j) * a.S] = ((wW * d[0] + wE * d[1]) + wS * d[2]) + wN * d[3];
  }
}

// the four scratch rows behind code c
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

// flux through one edge: left rows l, right rows r, c_e, k_e
__device__ __forceinline__ double edge_flux(const double l[ROWS], const double r[ROWS], double ce, const double k[3]) {
  const double ds = r[0] - l[0];
  const double g0 = l[1] + r[1], g1 = l[2] + r[2], g2 = l[3] + r[3];
  return ce * ds + 0.5 * ((g0 * k[0] + g1 * k[1]) + g2 * k[2]);
}

// MODE 0: store L; 1: the stage combination; 2: the stage combination and the accumulator
template <typename T, int MODE>
__global__ __launch_bounds__(256) void heat_flux_kernel(const KArgs a) {
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int n = a.n;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  int code[4];
  neighbours(a, t, x, y, c, code);
  double own[ROWS], nb[ROWS], k[3];
  load_rows(a, c, own);
  const size_t n1 = n + 1;
  // x-edge tables [T][n][n+1] (vectors: one plane per component), y-edge tables [T][n+1][n]
  const size_t ex = ((size_t)t * n + y) * n1 + x, px = (size_t)a.ntile * n * n1;
  const size_t ey = ((size_t)t * n1 + y) * n + x, py = (size_t)a.ntile * n1 * n;
  load_rows(a, code[0], nb);
  k[0] = a.kx[ex], k[1] = a.kx[px + ex], k[2] = a.kx[2 * px + ex];
  const double pW = edge_flux(nb, own, a.cx[ex], k);
  load_rows(a, code[1], nb);
  k[0] = a.kx[ex + 1], k[1] = a.kx[px + ex + 1], k[2] = a.kx[2 * px + ex + 1];
  const double pE = edge_flux(own, nb, a.cx[ex + 1], k);
  load_rows(a, code[2], nb);
  k[0] = a.ky[ey], k[1] = a.ky[py + ey], k[2] = a.ky[2 * py + ey];
  const double pS = edge_flux(nb, own, a.cy[ey], k);
  load_rows(a, code[3], nb);
  k[0] = a.ky[ey + n], k[1] = a.ky[py + ey + n], k[2] = a.ky[2 * py + ey + n];
  const double pN = edge_flux(own, nb, a.cy[ey + n], k);
  const double L = ((pE - pW) + (pN - pS)) * a.invA[((size_t)t * n + y) * n + x];
  if (MODE == 0) {
    a.lout[c] = L;
    return;
  }
  // the thread's own cell of X, Q and ACC, then its own cell of out and acc_out
  const double dq = a.kappa * L;
  const double xv = (MODE == 2 || a.a0 != 0.0) ? (double)((const T*)a.x)[c] : 0.0;
  double out = a.a2dt * dq;
  if (a.a1 != 0.0) out = out + a.a1 * (double)((const T*)a.q)[c];
  if (a.a0 != 0.0) out = out + a.a0 * xv;
  if (MODE == 2) {
    double acc = a.c1 * xv + a.c2dt * dq;
    if (a.acc_in && a.c0 != 0.0) acc = acc + a.c0 * (double)((const T*)a.acc_in)[c];
    ((T*)a.acc_out)[c] = (T)acc;
  }
  ((T*)a.out)[c] = (T)out;
}

template <typename T>
int launch(const HeatDesc* d, hipStream_t s) {
  KArgs a;
  a.q = d->q;
  a.recv = d->recv;
  a.scratch = d->scratch;
  a.srecv = d->srecv;
  a.gmap = d->gmap;
  a.W = d->W;
  a.cx = d->cx;
  a.cy = d->cy;
  a.kx = d->kx;
  a.ky = d->ky;
  a.invA = d->invA;
  a.x = d->x;
  a.acc_in = d->acc_in;
  a.out = d->out;
  a.acc_out = d->acc_out;
  a.lout = d->lout;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nbx = a.nby = (d->n + HB - 1) / HB;
  a.recv_stride = d->recv_stride;
  a.kappa = d->kappa;
  a.a0 = d->a0;
  a.a1 = d->a1;
  a.a2dt = d->a2dt;
  a.c0 = d->c0;
  a.c1 = d->c1;
  a.c2dt = d->c2dt;
  const dim3 grid(d->nblocks), block(256);
  if (d->pass_ == 1)
    hipLaunchKernelGGL((heat_gradient_kernel<T>), grid, block, 0, s, a);
  else if (d->mode == 0)
    hipLaunchKernelGGL((heat_flux_kernel<T, 0>), grid, block, 0, s, a);
  else if (d->mode == 1)
    hipLaunchKernelGGL((heat_flux_kernel<T, 1>), grid, block, 0, s, a);
  else
    hipLaunchKernelGGL((heat_flux_kernel<T, 2>), grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_heat_desc_size(void) { return (int)sizeof(HeatDesc); }

extern "C" int stsp_heat_launch(int dtype, const HeatDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || d->mg < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  const int nb = (d->n + HB - 1) / HB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->scratch || !d->gmap || !d->W || !d->cx || !d->cy || !d->kx || !d->ky || !d->invA) return 1;
  if (d->nrecv < 0) return 1;
  if (d->pass_ == 1) {
    if (!d->q || (d->nrecv > 0 && (!d->recv || d->recv_stride < 1))) return 1;
  } else if (d->pass_ == 2) {
    if (d->nrecv > 0 && !d->srecv) return 1;
    if (d->mode == 0) {
      if (!d->lout) return 1;
    } else if (d->mode == 1 || d->mode == 2) {
      if (!d->out || (d->a1 != 0.0 && !d->q) || ((d->a0 != 0.0 || d->mode == 2) && !d->x)) return 1;
      if (d->mode == 2 && !d->acc_out) return 1;
    } else {
      return 1;
    }
  } else {
    return 1;
  }
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
