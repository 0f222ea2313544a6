// Helmholtz solve on the device: (I - tau L) x = b with the consistent Laplacian L
// of heat_kernel.hip, by unpreconditioned BiCGStab (L is not symmetric: the
// least-squares gradient correction breaks the symmetry of the two-point part).
// ops/heat.py::HeatOperator.solve drives it; the PyTorch twin of the same
// recurrences is models/diffusion.py::helmholtz_bicgstab.
//
// No host in the loop.  rho, alpha, omega, beta, ||r||, ||b||, the flags and the
// iteration count live in a block of ten doubles on the device (HelmBlock); every
// kernel reads its scalars from there, and the host launches a chunk of k
// iterations, then copies the block's last 16 bytes (relative residual, flags,
// count) back once.  A fold kernel sets CONVERGED once ||r|| <= tol ||b|| and
// BREAKDOWN when a denominator is zero or a sum is not finite; every kernel of this
// file tests the flags first and returns, so the rest of a chunk leaves x, r and
// the scalars as they were.  Nothing waits and nothing polls.  (The gradient pass
// is heat_kernel.hip's and knows no flag: it rewrites the scratch, which nothing
// reads afterwards.)
//
// One iteration, 10 launches, all on the caller's stream:
//
//   1  gradient(p)     heat_gradient_kernel<double> on the work row p -> scratch
//   2  matvec<AP>      v = p - tau L p from the scratch; block sums of (rhat, v)
//   3  fold<ALPHA>     alpha = rho / (rhat, v)
//   4  s = r - alpha v
//   5  gradient(s)
//   6  matvec<AS>      t = s - tau L s; block sums of (t, s) and (t, t)
//   7  fold<OMEGA>     omega = (t, s) / (t, t)     ((t, t) == 0: s == 0, omega = 0)
//   8  x = (x + alpha p) + omega s;  r = s - omega t; block sums of (rhat, r), (r, r)
//   9  fold<BETA>      count, ||r||, the flags, beta = (rho' / rho) (alpha / omega), rho = rho'
//  10  p = r + beta (p - omega v)
//
// and the set-up, 3 launches: gradient(x), matvec<AX0> (r = b - (x - tau L x),
// rhat = p = r, block sums of (r, r) and (b, b)), fold<RHO0>.  What is folded:
// every inner product rides in the launch that produces its vector, the three
// stores of the set-up are one kernel, and the update of x shares a launch with
// the one of r.  What is not: a scalar needs every block's sum, so each fold is a
// grid-wide dependency, and without atomics or a resident grid that is a launch
// boundary; steps 4 and 10 need the scalar of the fold before them and feed the
// gradient pass after them, which reads neighbours and is not ours to change.
//
// The matvec is pass 2 of heat_kernel.hip with the same neighbour, gmap and
// scratch access: one thread per cell, one workgroup per 16 x 16 cell block of a
// tile, ragged at the tile end, every table read once per cell.  A ragged thread
// stays in the kernel with zero partials, because the reduction needs all four
// waves.  Inner products are area weighted, (u, w) = sum_i ((A_i u_i) w_i) with
// A_i = 1 / invA_i.  A block's sum has a fixed order: __shfl_down across each
// wave of 64 (offsets 32, 16, .., 1), then the four wave sums from LDS in wave
// order by thread 0, which writes one double per inner product to
// partials[k][block].  The fold is one workgroup of 256: thread j adds the
// partials j, j + 256, .. in ascending order, then a halving tree in LDS.  No
// atomics anywhere, so two solves of one system give the same bits.
//
// Work vectors are float64 rows in the padded layout of the state; only interior
// cells are read or written, a neighbour across a tile side comes through gmap
// (one rank without remote ghosts: every code is >= 0).  The kernels see float64
// only: the host copies b and x0 into the rows b and x (an fp32 state is converted
// by that copy) and copies x out once at the end (rounded once to the state's
// type).  All arithmetic is float64 and contraction is off in this file: every
// product and sum rounds on its own, in the association the twin writes down.
// Plain C++ and vector stores only.
#include <cstddef>

#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int HB = 16;          // block edge
constexpr int NT = HB * HB;     // threads
constexpr int ROWS = 4;         // scratch rows

enum Row { RX = 0, RR, RH, RP, RV, RS, RT, RB };
enum Matvec { AX0 = 0, AP, AS };              // which product a matvec launch forms
enum Fold { RHO0 = 0, ALPHA, OMEGA, BETA };   // which scalars a fold launch updates

// the scalar block; the host reads the last 16 bytes
struct HelmBlock {
  double rho, alpha, omega, beta, rnorm, bnorm, tol, spare;
  double relres;
  int flags, iters;
};
static_assert(sizeof(HelmBlock) == STSP_HELM_BLOCK * sizeof(double), "HelmBlock");
static_assert(offsetof(HelmBlock, relres) == STSP_HELM_RECORD * sizeof(double), "HelmBlock record");

struct HArgs {
  double* work;
  const double* scratch;
  const int* gmap;
  const double* cx;
  const double* cy;
  const double* kx;
  const double* ky;
  const double* invA;
  double* partials;
  HelmBlock* blk;
  int ntile, n, S, mg, pw, nb, nblocks;
  double tau, tol;
};

__device__ __forceinline__ double* row(const HArgs& a, int r) { return a.work + (size_t)r * (size_t)a.S; }

// (tile, x, y) of this thread's cell; false: outside the ragged block
__device__ __forceinline__ bool decode(const HArgs& a, int& t, int& x, int& y) {
  int blk = blockIdx.x;
  const int xb = blk % a.nb;
  blk /= a.nb;
  const int yb = blk % a.nb;
  t = blk / a.nb;
  x = xb * HB + (threadIdx.x & (HB - 1));
  y = yb * HB + (threadIdx.x >> 4);
  return x < a.n && y < a.n;
}

// the block's sums of p0 and p1 (np of them) to partials[k][block]; every thread of the block calls it
__device__ __forceinline__ void block_sums(const HArgs& a, double p0, double p1, int np, double (*s_w)[NT / 64]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    p0 = p0 + __shfl_down(p0, o, 64);
    p1 = p1 + __shfl_down(p1, o, 64);
  }
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
    s_w[0][tid >> 6] = p0;
    s_w[1][tid >> 6] = p1;
  }
  __syncthreads();
  if (tid == 0) {
    a.partials[blockIdx.x] = ((s_w[0][0] + s_w[0][1]) + s_w[0][2]) + s_w[0][3];
    if (np > 1) a.partials[(size_t)a.nblocks + blockIdx.x] = ((s_w[1][0] + s_w[1][1]) + s_w[1][2]) + s_w[1][3];
  }
}

// the four scratch rows of cell c
__device__ __forceinline__ void load_rows(const HArgs& a, int c, double r[ROWS]) {
  const double* q = a.scratch + c;
#pragma unroll
  for (int k = 0; k < ROWS; ++k) r[k] = q[(size_t)k * a.S];
}

// flux through one edge: left rows l, right rows r, c_e, k_e (heat_kernel.hip's)
__device__ __forceinline__ double edge_flux(const double l[ROWS], const double r[ROWS], double ce, const double k[3]) {
  const double ds = r[0] - l[0];
  const double g0 = l[1] + r[1], g1 = l[2] + r[2], g2 = l[3] + r[3];
  return ce * ds + 0.5 * ((g0 * k[0] + g1 * k[1]) + g2 * k[2]);
}

// u - tau L u of the vector u behind the scratch, at interior cell (t, x, y), padded offset c
__device__ __forceinline__ double helmholtz(const HArgs& a, int t, int x, int y, int c, double& u) {
  const int n = a.n;
  const int* g = a.gmap + (size_t)t * 4 * a.mg * n;
  const size_t side = (size_t)a.mg * n;
  const int cW = x > 0 ? c - 1 : g[y];
  const int cE = x < n - 1 ? c + 1 : g[side + y];
  const int cS = y > 0 ? c - a.pw : g[2 * side + x];
  const int cN = y < n - 1 ? c + a.pw : g[3 * side + x];
  double own[ROWS], nb[ROWS], k[3];
  load_rows(a, c, own);
  const size_t n1 = n + 1;
  const size_t ex = ((size_t)t * n + y) * n1 + x, px = (size_t)a.ntile * n * n1;
  const size_t ey = ((size_t)t * n1 + y) * n + x, py = (size_t)a.ntile * n1 * n;
  load_rows(a, cW, nb);
  k[0] = a.kx[ex], k[1] = a.kx[px + ex], k[2] = a.kx[2 * px + ex];
  const double pW = edge_flux(nb, own, a.cx[ex], k);
  load_rows(a, cE, nb);
  k[0] = a.kx[ex + 1], k[1] = a.kx[px + ex + 1], k[2] = a.kx[2 * px + ex + 1];
  const double pE = edge_flux(own, nb, a.cx[ex + 1], k);
  load_rows(a, cS, nb);
  k[0] = a.ky[ey], k[1] = a.ky[py + ey], k[2] = a.ky[2 * py + ey];
  const double pS = edge_flux(nb, own, a.cy[ey], k);
  load_rows(a, cN, nb);
  k[0] = a.ky[ey + n], k[1] = a.ky[py + ey + n], k[2] = a.ky[2 * py + ey + n];
  const double pN = edge_flux(own, nb, a.cy[ey + n], k);
  const double L = ((pE - pW) + (pN - pS)) * a.invA[((size_t)t * n + y) * n + x];
  u = own[0];
  return u - a.tau * L;
}

// AX0: r = b - A x, rhat = p = r, (r, r), (b, b);  AP: v = A p, (rhat, v);  AS: t = A s, (t, s), (t, t)
template <int MODE>
__global__ __launch_bounds__(NT) void helm_matvec_kernel(const HArgs a) {
  __shared__ double s_w[2][NT / 64];
  if (MODE != AX0 && a.blk->flags) return;
  int t, x, y;
  double p0 = 0.0, p1 = 0.0;
  if (decode(a, t, x, y)) {
    const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
    double u;
    const double au = helmholtz(a, t, x, y, c, u);
    const double area = 1.0 / a.invA[((size_t)t * a.n + y) * a.n + x];
    if (MODE == AX0) {
      const double b = row(a, RB)[c];
      const double r = b - au;
      row(a, RR)[c] = r;
      row(a, RH)[c] = r;
      row(a, RP)[c] = r;
      p0 = (area * r) * r;
      p1 = (area * b) * b;
    } else if (MODE == AP) {
      row(a, RV)[c] = au;
      p0 = (area * row(a, RH)[c]) * au;
    } else {
      row(a, RT)[c] = au;
      const double w = area * au;
      p0 = w * u;
      p1 = w * au;
    }
  }
  block_sums(a, p0, p1, MODE == AP ? 1 : 2, s_w);
}

// s = r - alpha v
__global__ __launch_bounds__(NT) void helm_s_kernel(const HArgs a) {
  if (a.blk->flags) return;
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  row(a, RS)[c] = row(a, RR)[c] - a.blk->alpha * row(a, RV)[c];
}

// x = (x + alpha p) + omega s, r = s - omega t, (rhat, r), (r, r)
__global__ __launch_bounds__(NT) void helm_xr_kernel(const HArgs a) {
  __shared__ double s_w[2][NT / 64];
  if (a.blk->flags) return;
  int t, x, y;
  double p0 = 0.0, p1 = 0.0;
  if (decode(a, t, x, y)) {
    const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
    const double alpha = a.blk->alpha, omega = a.blk->omega;
    const double s = row(a, RS)[c];
    row(a, RX)[c] = (row(a, RX)[c] + alpha * row(a, RP)[c]) + omega * s;
    const double r = s - omega * row(a, RT)[c];
    row(a, RR)[c] = r;
    const double area = 1.0 / a.invA[((size_t)t * a.n + y) * a.n + x];
    p0 = (area * row(a, RH)[c]) * r;
    p1 = (area * r) * r;
  }
  block_sums(a, p0, p1, 2, s_w);
}

// p = r + beta (p - omega v)
__global__ __launch_bounds__(NT) void helm_p_kernel(const HArgs a) {
  if (a.blk->flags) return;
  int t, x, y;
  if (!decode(a, t, x, y)) return;
  const int c = (t * a.pw + y + a.mg) * a.pw + x + a.mg;
  row(a, RP)[c] = row(a, RR)[c] + a.blk->beta * (row(a, RP)[c] - a.blk->omega * row(a, RV)[c]);
}

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }

// one workgroup: the partials in a fixed order, then the scalars of step WHICH
template <int WHICH>
__global__ __launch_bounds__(NT) void helm_fold_kernel(const HArgs a) {
  __shared__ double s_r[2][NT];
  HelmBlock* const k = a.blk;
  if (WHICH != RHO0 && k->flags) return;
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int b = tid; b < a.nblocks; b += NT) {
    a0 = a0 + a.partials[b];
    if (WHICH != ALPHA) a1 = a1 + a.partials[(size_t)a.nblocks + b];
  }
  s_r[0][tid] = a0;
  s_r[1][tid] = a1;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if (tid < h) {
      s_r[0][tid] = s_r[0][tid] + s_r[0][tid + h];
      s_r[1][tid] = s_r[1][tid] + s_r[1][tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  const double s0 = s_r[0][0], s1 = s_r[1][0];
  if (WHICH == RHO0) {              // s0 = (r, r) = (rhat, r), s1 = (b, b)
    k->rho = s0;
    k->alpha = k->omega = k->beta = k->spare = 0.0;
    k->tol = a.tol;
    k->rnorm = sqrt(s0);
    k->bnorm = sqrt(s1);
    k->relres = k->bnorm > 0.0 ? k->rnorm / k->bnorm : k->rnorm;
    k->iters = 0;
    k->flags = !(finite(s0) && finite(s1)) ? STSP_HELM_BREAKDOWN
                                            : (k->rnorm <= a.tol * k->bnorm ? STSP_HELM_CONVERGED : 0);
  } else if (WHICH == ALPHA) {      // s0 = (rhat, v)
    if (s0 == 0.0 || !finite(s0) || !finite(k->rho)) k->flags = STSP_HELM_BREAKDOWN;
    else k->alpha = k->rho / s0;
  } else if (WHICH == OMEGA) {      // s0 = (t, s), s1 = (t, t)
    if (!finite(s0) || !finite(s1)) k->flags = STSP_HELM_BREAKDOWN;
    else k->omega = s1 == 0.0 ? 0.0 : s0 / s1;
  } else {                          // s0 = (rhat, r), s1 = (r, r); x and r are those of the finished iteration
    k->iters = k->iters + 1;
    k->rnorm = sqrt(s1);
    k->relres = k->bnorm > 0.0 ? k->rnorm / k->bnorm : k->rnorm;
    if (!finite(s0) || !finite(s1)) {
      k->flags = STSP_HELM_BREAKDOWN;
    } else if (k->rnorm <= k->tol * k->bnorm) {
      k->flags = STSP_HELM_CONVERGED;
    } else if (k->rho == 0.0 || k->omega == 0.0) {
      k->flags = STSP_HELM_BREAKDOWN;
    } else {
      k->beta = (s0 / k->rho) * (k->alpha / k->omega);
      k->rho = s0;
    }
  }
}

// pass 1 of heat_kernel.hip on work row r: the row and its gradient into the scratch
int gradient(const HelmDesc* d, int r, hipStream_t s) {
  HeatDesc h = {};
  h.q = d->work + (size_t)r * (size_t)d->S;
  h.scratch = d->scratch;
  h.gmap = d->gmap;
  h.W = d->W;
  h.cx = d->cx;
  h.cy = d->cy;
  h.kx = d->kx;
  h.ky = d->ky;
  h.invA = d->invA;
  h.ntile = d->ntile;
  h.n = d->n;
  h.S = d->S;
  h.mg = d->mg;
  h.pw = d->pw;
  h.nrecv = 0;
  h.recv_stride = 1;
  h.nblocks = d->nblocks;
  h.pass_ = 1;
  return stsp_heat_launch(1, &h, s);
}

#define HELM_LAUNCH(kernel, blocks)                                   \
  do {                                                                \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(NT), 0, s, a);      \
    if (hipGetLastError() != hipSuccess) return 3;                    \
  } while (0)

int launch(const HelmDesc* d, hipStream_t s) {
  HArgs a;
  a.work = d->work;
  a.scratch = d->scratch;
  a.gmap = d->gmap;
  a.cx = d->cx;
  a.cy = d->cy;
  a.kx = d->kx;
  a.ky = d->ky;
  a.invA = d->invA;
  a.partials = d->partials;
  a.blk = (HelmBlock*)d->block;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nb = (d->n + HB - 1) / HB;
  a.nblocks = d->nblocks;
  a.tau = d->tau;
  a.tol = d->tol;
  int rc;
  if (d->op == 0) {
    if ((rc = gradient(d, RX, s)) != 0) return rc;
    HELM_LAUNCH(helm_matvec_kernel<AX0>, d->nblocks);
    HELM_LAUNCH(helm_fold_kernel<RHO0>, 1);
    return 0;
  }
  for (int it = 0; it < d->iters; ++it) {
    if ((rc = gradient(d, RP, s)) != 0) return rc;
    HELM_LAUNCH(helm_matvec_kernel<AP>, d->nblocks);
    HELM_LAUNCH(helm_fold_kernel<ALPHA>, 1);
    HELM_LAUNCH(helm_s_kernel, d->nblocks);
    if ((rc = gradient(d, RS, s)) != 0) return rc;
    HELM_LAUNCH(helm_matvec_kernel<AS>, d->nblocks);
    HELM_LAUNCH(helm_fold_kernel<OMEGA>, 1);
    HELM_LAUNCH(helm_xr_kernel, d->nblocks);
    HELM_LAUNCH(helm_fold_kernel<BETA>, 1);
    HELM_LAUNCH(helm_p_kernel, d->nblocks);
  }
  return 0;
}

}  // namespace

extern "C" int stsp_helmholtz_desc_size(void) { return (int)sizeof(HelmDesc); }

// 1: a descriptor that does not describe a solve; 3: launch error
extern "C" int stsp_helmholtz_launch(const HelmDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || d->mg < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  const int nb = (d->n + HB - 1) / HB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->work || !d->scratch || !d->gmap || !d->W || !d->cx || !d->cy || !d->kx || !d->ky || !d->invA) return 1;
  if (!d->partials || !d->block) return 1;
  if (d->op == 0) {
    if (!(d->tol >= 0.0)) return 1;
  } else if (d->op == 1) {
    if (d->iters < 1 || d->iters > STSP_HELM_MAX_ITERS) return 1;
  } else {
    return 1;
  }
  if (!(d->tau - d->tau == 0.0)) return 1;
  return launch(d, stream);
}
