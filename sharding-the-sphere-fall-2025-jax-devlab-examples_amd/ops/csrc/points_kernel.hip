// Point sampling and Lagrangian particles on the device.  The definitions are
// those of models/points.py (the twin) and models/latlon.py::locate_points: a
// point p (unit vector, fp64 whatever the state's type) is located on the dual
// mesh of the cell centres, which gives four source cells and four fp64
// weights; the state's values are converted to fp64 and every sum is
// ((t0 + t1) + t2) + t3 with t = w x.
//
// Ordinary launches on the caller's stream, one thread per point, 256-thread
// workgroups, ragged tail; no atomics, no polling, nothing persistent, no LDS.
//
//  locate   panel = the largest of the six normal components (ties: the lowest
//           panel); x, y = the two atans in cell units; a coordinate within
//           1e-12 of an integer is that integer.  Inside the border centres:
//           the interior quad (ceil - 1: a point on a dual grid line goes to
//           the lower quad), bilinear weights.  In the border band: up to seven
//           candidates (three edge quads per side the point is beyond, the
//           nearest corner triangle), visited in ascending id without
//           repeats; edge quad: 12 Newton iterations from (1/2, 1/2) on the
//           inverse bilinear map in the gnomonic plane tangent at the point;
//           triangle: barycentric weights; the lowest id whose inside measure
//           is >= -1e-12 wins (none: the largest measure).
//  sample   scalar mode: C channels of stride cs; velocity mode: v = M / h per
//           source cell (h == 0: M itself), three Cartesian components.  A cell
//           the rank does not own (map -1) contributes 0 and reads nothing.
//           Output [C][K], or the four terms of every sum [C][4][K] (several
//           ranks add these arrays, one rank owns each term, and the advance
//           launch folds them in the one-rank association).
//  advance  corrector x <- move(x, dtp/2 (v0 + v1)), v1 the tangent part at xs
//           of the velocity sampled there; predictor v0 <- tangent part at x of
//           the velocity sampled there, xs <- move(x, dtp v0).
//  fused    one rank: sample at xs, corrector, sample at x, predictor in one
//           thread; the same device functions, so the positions equal the
//           sample / advance sequence bit for bit.
//
// Contract (what keeps every address inside the tables and the state):
//  * every table index is clamped to its table's range before use: panel 0..5,
//    side 0..3, position 0..N-2 into eid; eid's values to 0..12(N-1)-1 and
//    ctri's to 0..7 before they index bcell / bctr; cell ids to 0..6NN-1 before
//    they index cmap; cmap's values to 0..lim-1 (lim <= cs) before they index a
//    channel.  Doubles are clamped as doubles before they become ints (a NaN
//    becomes the lower limit).
//  * a point that is not finite returns early with NaN outputs (elem -1) and
//    reads no table and no state.  In the advance kernels a non-finite position
//    needs no branch: the arithmetic keeps it NaN ("lost").
//
// Contraction is off in this file: every product and sum rounds on its own, in
// the association models/points.py writes down.
#include "stsp_kernels.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int LB = 256;
constexpr double TOL = 1e-12;   // models/latlon.py::CONTAIN_TOL

struct Loc {
  int g[4];       // global cell ids
  double w[4];
  int elem;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// clamp as a double, then convert: NaN -> lo
__device__ __forceinline__ int clampd(double v, int lo, int hi) { return (int)fmin(fmax(v, (double)lo), (double)hi); }
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// weights and inside measure of the point p in border element e (a row of bcell / bctr)
__device__ __forceinline__ void element_weights(const PointsDesc& d, int e, const double* p, const double* e1,
                                                const double* e2, double* w, double& ins, int* cells) {
  const int* bc = d.bcell + 4 * (size_t)e;
  const double* ctr = d.bctr + 12 * (size_t)e;
  cells[0] = bc[0]; cells[1] = bc[1]; cells[2] = bc[2]; cells[3] = bc[3];
  const bool tri = cells[3] < 0;
  double P[4][2];
  bool ok = true;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const double v[3] = {ctr[3 * m], ctr[3 * m + 1], ctr[3 * m + 2]};
    const double dd = dot3(v, p);
    const bool okm = dd > 1e-3;
    ok = ok && okm;
    const double den = okm ? dd : 1.0;
    const double g[3] = {v[0] / den, v[1] / den, v[2] / den};
    P[m][0] = dot3(g, e1);
    P[m][1] = dot3(g, e2);
  }
  if (tri) {
    const double bax = P[1][0] - P[0][0], bay = P[1][1] - P[0][1];
    const double cax = P[2][0] - P[0][0], cay = P[2][1] - P[0][1];
    const double nax = -P[0][0], nay = -P[0][1];
    double area = bax * cay - bay * cax;
    area = area == 0.0 ? 1.0 : area;
    const double w1 = (nax * cay - nay * cax) / area;
    const double w2 = (bax * nay - bay * nax) / area;
    const double w0 = (1.0 - w1) - w2;
    w[0] = w0; w[1] = w1; w[2] = w2; w[3] = 0.0;
    ins = fmin(w0, fmin(w1, w2));
    cells[3] = cells[0];
  } else {
    const double Ax = P[0][0], Ay = P[0][1];
    const double Bx = P[1][0] - P[0][0], By = P[1][1] - P[0][1];
    const double Cx = P[2][0] - P[0][0], Cy = P[2][1] - P[0][1];
    const double Dx = ((P[0][0] - P[1][0]) - P[2][0]) + P[3][0], Dy = ((P[0][1] - P[1][1]) - P[2][1]) + P[3][1];
    double s = 0.5, t = 0.5;
    for (int it = 0; it < 12; ++it) {
      const double st = s * t;
      const double rx = ((Ax + Bx * s) + Cx * t) + Dx * st, ry = ((Ay + By * s) + Cy * t) + Dy * st;
      const double jsx = Bx + Dx * t, jsy = By + Dy * t;
      const double jtx = Cx + Dx * s, jty = Cy + Dy * s;
      double det = jsx * jty - jsy * jtx;
      det = det == 0.0 ? 1.0 : det;
      s = s - (rx * jty - ry * jtx) / det;
      t = t - (jsx * ry - jsy * rx) / det;
    }
    w[0] = (1.0 - s) * (1.0 - t); w[1] = s * (1.0 - t); w[2] = (1.0 - s) * t; w[3] = s * t;
    ins = fmin(fmin(s, 1.0 - s), fmin(t, 1.0 - t));
  }
  if (!ok) ins = -INFINITY;
}

// location of a finite point (models/latlon.py::locate_points)
__device__ __forceinline__ void locate(const PointsDesc& d, const double* p, Loc& L) {
  const int N = d.N, nq = 12 * (N - 1);
  const double dn[6] = {p[2], p[1], -p[0], -p[1], p[0], -p[2]};
  int f = 0;
  double best = dn[0];
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (dn[k] > best) { best = dn[k]; f = k; }
  // (n, e_i, e_j) of the panel: parallel/topology.py::FACE_FRAMES
  double a, b;
  switch (f) {
    case 0: a = p[0]; b = p[1]; break;
    case 1: a = -p[0]; b = p[2]; break;
    case 2: a = -p[1]; b = p[2]; break;
    case 3: a = p[0]; b = p[2]; break;
    case 4: a = p[1]; b = p[2]; break;
    default: a = -p[0]; b = p[1]; break;
  }
  const double q = 0.25 * 3.141592653589793;
  double x = (atan(a / best) + q) / d.da - 0.5;
  double y = (atan(b / best) + q) / d.da - 0.5;
  const double rx = rint(x), ry = rint(y);
  if (fabs(x - rx) <= TOL) x = rx;
  if (fabs(y - ry) <= TOL) y = ry;
  const bool xlo = x < 0.0, xhi = x > (double)(N - 1), ylo = y < 0.0, yhi = y > (double)(N - 1);
  if (!(xlo || xhi || ylo || yhi)) {
    const int i0 = clampd(ceil(x) - 1.0, 0, N - 2), j0 = clampd(ceil(y) - 1.0, 0, N - 2);
    const double tx = x - (double)i0, ty = y - (double)j0;
    const int c = (f * N + j0) * N + i0;
    L.g[0] = c; L.g[1] = c + 1; L.g[2] = c + N; L.g[3] = c + N + 1;
    L.w[0] = (1.0 - tx) * (1.0 - ty); L.w[1] = tx * (1.0 - ty); L.w[2] = (1.0 - tx) * ty; L.w[3] = tx * ty;
    L.elem = (f * (N - 1) + j0) * (N - 1) + i0;
    return;
  }
  // border band
  const int jy = clampd(floor(y), 0, N - 2), jx = clampd(floor(x), 0, N - 2);
  const int xs = xhi ? 1 : 0, ys = yhi ? 3 : 2;
  const bool bx = xlo || xhi, by = ylo || yhi;
  int cand[7];
#pragma unroll
  for (int o = -1; o <= 1; ++o) {
    cand[1 + o] = bx ? clampi(d.eid[(f * 4 + xs) * (N - 1) + clampi(jy + o, 0, N - 2)], 0, nq - 1) : -1;
    cand[4 + o] = by ? clampi(d.eid[(f * 4 + ys) * (N - 1) + clampi(jx + o, 0, N - 2)], 0, nq - 1) : -1;
  }
  const double half = 0.5 * (double)(N - 1);
  cand[6] = nq + clampi(d.ctri[f * 4 + (x > half ? 1 : 0) + (y > half ? 2 : 0)], 0, 7);
  // tangent basis at p
  double e1[3], e2[3];
  if (fabs(p[0]) < 0.9) { e1[0] = 0.0; e1[1] = -p[2]; e1[2] = p[1]; }
  else { e1[0] = p[2]; e1[1] = 0.0; e1[2] = -p[0]; }
  const double n1 = sqrt(dot3(e1, e1));
  e1[0] /= n1; e1[1] /= n1; e1[2] /= n1;
  e2[0] = p[1] * e1[2] - p[2] * e1[1];
  e2[1] = p[2] * e1[0] - p[0] * e1[2];
  e2[2] = p[0] * e1[1] - p[1] * e1[0];
  double ins = -INFINITY;
  int last = -1;
  L.elem = 6 * (N - 1) * (N - 1);
  L.g[0] = L.g[1] = L.g[2] = L.g[3] = 0;
  L.w[0] = L.w[1] = L.w[2] = L.w[3] = 0.0;
  for (int it = 0; it < 7; ++it) {
    int e = 0x7fffffff;       // the lowest candidate above the last one visited
#pragma unroll
    for (int c = 0; c < 7; ++c)
      if (cand[c] > last && cand[c] < e) e = cand[c];
    if (e == 0x7fffffff) break;
    last = e;
    double w[4], ic;
    int cells[4];
    element_weights(d, e, p, e1, e2, w, ic, cells);
    if (ic > ins) {
      ins = ic;
      L.elem = 6 * (N - 1) * (N - 1) + e;
#pragma unroll
      for (int s = 0; s < 4; ++s) { L.w[s] = w[s]; L.g[s] = cells[s]; }
    }
    if (ic >= -TOL) break;
  }
}

// index of global cell g inside a channel, -1 = not owned; both table accesses clamped
__device__ __forceinline__ long long cell_index(const PointsDesc& d, int g) {
  const int i = d.cmap[clampi(g, 0, 6 * d.N * d.N - 1)];
  if (i < 0) return -1;
  return (long long)i < d.lim ? (long long)i : d.lim - 1;
}

// the four velocity terms per component at a finite point
template <typename T>
__device__ __forceinline__ void velocity_terms(const PointsDesc& d, const double* p, double t[4][3], int* elem) {
  Loc L;
  locate(d, p, L);
  if (elem) *elem = L.elem;
  const T* Q = (const T*)d.Q;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    t[s][0] = t[s][1] = t[s][2] = 0.0;
    const long long c = cell_index(d, L.g[s]);
    if (c >= 0) {
      const double h = (double)Q[c];
      const double den = h != 0.0 ? h : 1.0;
      t[s][0] = L.w[s] * ((double)Q[d.cs + c] / den);
      t[s][1] = L.w[s] * ((double)Q[2 * d.cs + c] / den);
      t[s][2] = L.w[s] * ((double)Q[3 * d.cs + c] / den);
    }
  }
}

// folded velocity at p; NaN for a point that is not finite
template <typename T>
__device__ __forceinline__ void velocity_at(const PointsDesc& d, const double* p, double* v) {
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
    v[0] = v[1] = v[2] = NAN;
    return;
  }
  double t[4][3];
  velocity_terms<T>(d, p, t, nullptr);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((t[0][c] + t[1][c]) + t[2][c]) + t[3][c];
}

__device__ __forceinline__ void tangent(const double* v, const double* x, double* out) {
  const double s = dot3(v, x);
  out[0] = v[0] - s * x[0]; out[1] = v[1] - s * x[1]; out[2] = v[2] - s * x[2];
}

// x carried along the great circle of the tangent part of dsp (m)
__device__ __forceinline__ void move(const double* x, const double* dsp, double radius, double* out) {
  double e[3];
  tangent(dsp, x, e);
  const double n = sqrt(dot3(e, e));
  if (n == 0.0) {
    out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
    return;
  }
  const double th = n / radius;
  const double c = cos(th), s = sin(th);
  double y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = c * x[k] + s * (e[k] / n);
  const double ny = sqrt(dot3(y, y));
  out[0] = y[0] / ny; out[1] = y[1] / ny; out[2] = y[2] / ny;
}

// x <- move(x, dtp/2 (v0 + v1)), v1 the tangent part at xs of v
__device__ __forceinline__ void corrector(const PointsDesc& d, const double* v, const double* xs, const double* v0,
                                          double* x) {
  double v1[3], dsp[3], xn[3];
  tangent(v, xs, v1);
  const double hd = 0.5 * d.dtp;
#pragma unroll
  for (int k = 0; k < 3; ++k) dsp[k] = hd * (v0[k] + v1[k]);
  move(x, dsp, d.radius, xn);
  x[0] = xn[0]; x[1] = xn[1]; x[2] = xn[2];
}

// v0 <- tangent part at x of v; xs <- move(x, dtp v0)
__device__ __forceinline__ void predictor(const PointsDesc& d, const double* v, const double* x, double* v0,
                                          double* xs) {
  double dsp[3];
  tangent(v, x, v0);
#pragma unroll
  for (int k = 0; k < 3; ++k) dsp[k] = d.dtp * v0[k];
  move(x, dsp, d.radius, xs);
}

__device__ __forceinline__ void load3(const double* a, size_t k, double* v) {
  v[0] = a[3 * k]; v[1] = a[3 * k + 1]; v[2] = a[3 * k + 2];
}
__device__ __forceinline__ void store3(double* a, size_t k, const double* v) {
  a[3 * k] = v[0]; a[3 * k + 1] = v[1]; a[3 * k + 2] = v[2];
}

template <typename T>
__global__ __launch_bounds__(LB) void points_sample_kernel(const PointsDesc d) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= d.K) return;
  const size_t K = (size_t)d.K;
  double p[3];
  load3(d.p, (size_t)k, p);
  const int rows = d.terms ? 4 * d.C : d.C;
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) {
    for (int r = 0; r < rows; ++r) d.out[(size_t)r * K + k] = NAN;
    if (d.elem) d.elem[k] = -1;
    return;
  }
  if (d.velocity) {
    double t[4][3];
    int el;
    velocity_terms<T>(d, p, t, &el);
    if (d.elem) d.elem[k] = el;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (d.terms) {
#pragma unroll
        for (int s = 0; s < 4; ++s) d.out[(size_t)(4 * c + s) * K + k] = t[s][c];
      } else {
        d.out[(size_t)c * K + k] = ((t[0][c] + t[1][c]) + t[2][c]) + t[3][c];
      }
    }
    return;
  }
  Loc L;
  locate(d, p, L);
  if (d.elem) d.elem[k] = L.elem;
  long long ci[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) ci[s] = cell_index(d, L.g[s]);
  for (int c = 0; c < d.C; ++c) {
    const T* q = (const T*)d.Q + (size_t)c * (size_t)d.cs;
    double t[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = ci[s] >= 0 ? L.w[s] * (double)q[ci[s]] : 0.0;
    if (d.terms) {
#pragma unroll
      for (int s = 0; s < 4; ++s) d.out[(size_t)(4 * c + s) * K + k] = t[s];
    } else {
      d.out[(size_t)c * K + k] = ((t[0] + t[1]) + t[2]) + t[3];
    }
  }
}

__global__ __launch_bounds__(LB) void points_advance_kernel(const PointsDesc d) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= d.K) return;
  const size_t K = (size_t)d.K;
  double v[3], x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (d.terms) {
      const double* q = d.vel + (size_t)(4 * c) * K + k;
      v[c] = ((q[0] + q[K]) + q[2 * K]) + q[3 * K];
    } else {
      v[c] = d.vel[(size_t)c * K + k];
    }
  }
  load3(d.x, (size_t)k, x);
  if (d.stage == 0) {
    double xs[3], v0[3];
    load3(d.xs, (size_t)k, xs);
    load3(d.v0, (size_t)k, v0);
    corrector(d, v, xs, v0, x);
    store3(d.x, (size_t)k, x);
  } else {
    double xs[3], v0[3];
    predictor(d, v, x, v0, xs);
    store3(d.v0, (size_t)k, v0);
    store3(d.xs, (size_t)k, xs);
  }
}

template <typename T>
__global__ __launch_bounds__(LB) void points_fused_kernel(const PointsDesc d) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= d.K) return;
  double x[3], xs[3], v0[3], v[3];
  load3(d.x, (size_t)k, x);
  load3(d.xs, (size_t)k, xs);
  load3(d.v0, (size_t)k, v0);
  velocity_at<T>(d, xs, v);
  corrector(d, v, xs, v0, x);
  velocity_at<T>(d, x, v);
  predictor(d, v, x, v0, xs);
  store3(d.x, (size_t)k, x);
  store3(d.v0, (size_t)k, v0);
  store3(d.xs, (size_t)k, xs);
}

template <typename T>
int launch(const PointsDesc* d, hipStream_t s) {
  const dim3 grid((d->K + LB - 1) / LB), block(LB);
  if (d->mode == 0)
    hipLaunchKernelGGL(points_sample_kernel<T>, grid, block, 0, s, *d);
  else if (d->mode == 1)
    hipLaunchKernelGGL(points_advance_kernel, grid, block, 0, s, *d);
  else
    hipLaunchKernelGGL(points_fused_kernel<T>, grid, block, 0, s, *d);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_points_desc_size(void) { return (int)sizeof(PointsDesc); }

extern "C" int stsp_points_launch(int dtype, const PointsDesc* d, hipStream_t stream) {
  if (!d || d->K <= 0 || d->K > 2147483392 || d->mode < 0 || d->mode > 2) return 1;
  if (d->mode != 1) {      // the launches that locate
    if (d->N < 2 || d->N > 16384 || !d->Q || !d->cmap || !d->eid || !d->bcell || !d->ctri || !d->bctr) return 1;
    if (d->cs <= 0 || d->lim <= 0 || d->lim > d->cs || !(d->da > 0.0)) return 1;
  }
  if (d->mode == 0) {
    if (!d->p || !d->out || d->C <= 0 || (d->velocity && d->C != 3)) return 1;
  } else {
    if (!d->x || !d->xs || !d->v0 || !(d->radius > 0.0) || !(d->dtp == d->dtp)) return 1;
    if (d->mode == 1 && (!d->vel || d->stage < 0 || d->stage > 1)) return 1;
  }
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
