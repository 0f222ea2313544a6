// Time-dependent winds of the advection model on the device: the edge-transport
// tables ex [T][n][n+1] and ey [T][n+1][n] that the stage kernel (physics 0)
// reads, refilled in place before every Runge-Kutta stage (the twin:
// models/advection.py::Advection.transports; the flows:
// models/initial_conditions.py).
//
// The time lives on the device.  A launch takes dt, the stage's abscissa c_s and
// a pointer to the step count and forms
//     t_s = ((double)count + c_s) * dt
// itself, two roundings as the host forms (step_count + c_s) * dt; a one-thread
// tick launch adds one to the count at the end of a step.  A captured graph of k
// steps therefore evaluates k different winds on every replay.
//
//  mode 0  streamfunction flows (deform_nd, deform_nd_static).  With lam' = lam - w t,
//            psi = P sin^2(lam') c(t) + Q,    c(t) = cos(pi t / T),
//            sin(lam') = sin(lam) cos(w t) - cos(lam) sin(w t),
//          from the vertex table vtab [4][T][n+1][n+1] = sin lam, cos lam,
//          P = R k cos^2 th, Q = -R u_rot sin th.  The transport through an edge is
//          the difference of psi at its two vertices,
//            x-edge (j, i): U = -(psi[j+1][i] - psi[j][i])
//            y-edge (j, i): U = +(psi[j][i+1] - psi[j][i]),
//          so a cell's four transports sum to zero to rounding.  One workgroup per
//          16 x 16 cell block of a tile (ragged at the tile end): psi once per
//          vertex of the block's 17 x 17 patch into LDS, then each thread stores the
//          west and south edge of its cell, and the east / north edge too where its
//          cell is the tile's last column / row.
//  mode 1  the divergent flow (deform_div): the midpoint rule U = (v . m) L with
//            U = c(t) [A (1 - cos lam') + B sin lam'] + C
//          from the edge tables xtab [5][T][n][n+1], ytab [5][T][n+1][n] = sin lam,
//          cos lam of the midpoint, A = -(k / 2) sin 2th cos^2 th (e . m) L,
//          B = (k / 2) cos^3 th (n . m) L, C = u_rot cos th (e . m) L; sin^2(lam'/2) =
//          (1 - cos lam') / 2.  One thread per edge, the x-edges first.
//
// Both modes need the sine and cosine of w t and cos(pi t / T) only: thread 0
// computes them once per workgroup and hands them over in LDS.  Every table is
// float64 and so is all arithmetic; the result is rounded once to the tables'
// element type.  Contraction is off in this file.  Plain C++ and vector stores
// only; no atomics, nothing persistent.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int WB = 16;          // block edge (cells)
constexpr int WP = WB + 1;      // vertices per patch edge

struct Trig {
  double sw, cw, ct;            // sin(w t), cos(w t), cos(pi t / T)
};

__device__ __forceinline__ void stage_trig(const WindDesc& d, double* sh) {
  if (threadIdx.x == 0) {
    const double t = ((double)d.count[0] + d.cs) * d.dt;
    double s, c;
    sincos(d.omega * t, &s, &c);
    sh[0] = s;
    sh[1] = c;
    sh[2] = cos(d.pi_over_T * t);
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void wind_stream_kernel(const WindDesc d) {
  __shared__ double trig[3];
  __shared__ double psi[WP][WP];
  stage_trig(d, trig);
  const Trig g = {trig[0], trig[1], trig[2]};
  const int n = d.n, n1 = n + 1;
  const int nb = (n + WB - 1) / WB;
  int blk = blockIdx.x;
  const int xb = blk % nb;
  blk /= nb;
  const int yb = blk % nb;
  const int t = blk / nb;                       // < ntile: nblocks = ntile * nb * nb, checked at launch
  const int x0 = xb * WB, y0 = yb * WB;
  const size_t plane = (size_t)d.ntile * n1 * n1;
  const double* vt = d.vtab + (size_t)t * n1 * n1;
  for (int k = threadIdx.x; k < WP * WP; k += 256) {
    const int py = k / WP, px = k - py * WP;
    const int vx = x0 + px, vy = y0 + py;
    if (vx <= n && vy <= n) {
      const size_t v = (size_t)vy * n1 + vx;
      const double sl = vt[v], cl = vt[plane + v], P = vt[2 * plane + v], Q = vt[3 * plane + v];
      const double s = sl * g.cw - cl * g.sw;
      psi[py][px] = (P * (s * s)) * g.ct + Q;
    }
  }
  __syncthreads();
  const int tx = threadIdx.x & (WB - 1), ty = threadIdx.x >> 4;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= n || y >= n) return;
  T* ex = (T*)d.ex + ((size_t)t * n + y) * n1 + x;     // x-edge (y, x), x <= n
  T* ey = (T*)d.ey + ((size_t)t * n1 + y) * n + x;     // y-edge (y, x), y <= n
  const double p00 = psi[ty][tx], p10 = psi[ty + 1][tx], p01 = psi[ty][tx + 1];
  ex[0] = (T)(-(p10 - p00));
  ey[0] = (T)(p01 - p00);
  if (x == n - 1 || y == n - 1) {
    const double p11 = psi[ty + 1][tx + 1];
    if (x == n - 1) ex[1] = (T)(-(p11 - p01));
    if (y == n - 1) ey[n] = (T)(p11 - p10);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void wind_edge_kernel(const WindDesc d) {
  __shared__ double trig[3];
  stage_trig(d, trig);
  const Trig g = {trig[0], trig[1], trig[2]};
  const size_t ne = (size_t)d.ntile * d.n * (d.n + 1);        // x-edges; as many y-edges
  size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * ne) return;
  const double* tab = d.xtab;
  T* out = (T*)d.ex;
  if (e >= ne) {
    e -= ne;
    tab = d.ytab;
    out = (T*)d.ey;
  }
  const double sl = tab[e], cl = tab[ne + e], A = tab[2 * ne + e], B = tab[3 * ne + e], C = tab[4 * ne + e];
  const double s = sl * g.cw - cl * g.sw;       // sin lam'
  const double c = cl * g.cw + sl * g.sw;       // cos lam'
  out[e] = (T)((A * (1.0 - c) + B * s) * g.ct + C);
}

__global__ void wind_tick_kernel(int* count) { count[0] = count[0] + 1; }

template <typename T>
int launch(const WindDesc* d, hipStream_t s) {
  if (d->mode == 0)
    hipLaunchKernelGGL((wind_stream_kernel<T>), dim3(d->nblocks), dim3(256), 0, s, *d);
  else
    hipLaunchKernelGGL((wind_edge_kernel<T>), dim3(d->nblocks), dim3(256), 0, s, *d);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_wind_desc_size(void) { return (int)sizeof(WindDesc); }

extern "C" int stsp_wind_launch(int dtype, const WindDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || !d->ex || !d->ey || !d->count) return 1;
  const long long nb = (d->n + WB - 1) / WB;
  const long long ne = (long long)d->ntile * d->n * (d->n + 1);
  if (ne >= (1LL << 30)) return 1;
  if (d->mode == 0) {
    if (!d->vtab || (long long)d->nblocks != d->ntile * nb * nb) return 1;
  } else if (d->mode == 1) {
    if (!d->xtab || !d->ytab || (long long)d->nblocks != (2 * ne + 255) / 256) return 1;
  } else {
    return 1;
  }
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}

extern "C" int stsp_wind_tick(int* count, hipStream_t stream) {
  if (!count) return 1;
  hipLaunchKernelGGL(wind_tick_kernel, dim3(1), dim3(1), 0, stream, count);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
