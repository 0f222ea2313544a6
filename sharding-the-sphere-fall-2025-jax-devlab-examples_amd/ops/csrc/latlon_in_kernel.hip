// Lat-lon input on the device: the padded state of a rank from gridded h, u, v
// and scalars.  The inverse direction of latlon_kernel.hip; the definitions and
// the numpy twin are models/latlon_in.py.
//
// Two ordinary launches on the caller's stream, nothing persistent, no atomics:
//
//  prepare  one 256-thread workgroup per source latitude row.  It converts the
//           input channels (fp32 or fp64) to the float64 work copy
//           [C][nlat][nlon] and forms Vx, Vy, Vz from (u, v): one sincos per
//           longitude, the row's sincos(lat) once.  On a pole row the vectors go
//           through LDS in chunks of PCH longitudes and threads 0 .. 2 carry the
//           running sum of one component each in ascending longitude, so the
//           association is ((V_0 + V_1) + V_2) + ... whatever nlon is; the mean is
//           broadcast through LDS and written over the row.
//  ingest   the rank's own cells in 16 x 16 blocks of a tile (ragged for any n),
//           q q lanes per cell (1, 4 or 16: a wave serves 64, 16 or 4 cells), so a
//           block is q q workgroups of 256 threads, each 16 / (q q) ... 16 rows of
//           it.  A lane derives its Gauss point from (tile, j, i) and the tile's
//           (panel, I0, J0) in float64: alpha = ((2 I + 1 - N) + g) dalpha / 2, the
//           gnomonic map, lat = asin, lon = atan2.  It computes the base indices and
//           the 2 or 4 + 2 or 4 tap weights once, resolves the wrap and the pole
//           reflection on the row indices (with the row's column shift nlon / 2)
//           and the column indices, not per tap, and reuses them for every
//           channel (up to 8, in registers).  The lanes of a cell are folded by a
//           fixed __shfl_xor butterfly (1, 2, 4, 8), together with the weights, so
//           the result does not depend on the launch shape.  Lane 0 of the cell
//           divides, projects V onto the tangent plane at the cell centre, forms
//           M = h V_t and hq_k = h q_k and stores into the interior of the padded
//           state [F][S] in the state's type.  Ghost slots are not written here.
//
// All arithmetic is float64 with contraction off: every product and sum rounds
// on its own, in the association the twin writes down.  `order` and `q` are
// template parameters; the channel count is a launch value.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LB = 256;     // workgroup size of both kernels
constexpr int BLK = 16;     // cells per block edge
constexpr int PCH = 1024;   // longitudes of a pole row folded per LDS pass
constexpr int MAXC = 8;     // work channels

__constant__ int FRAMES[6][9] = {
    {0, 0, 1, 1, 0, 0, 0, 1, 0},  {0, 1, 0, -1, 0, 0, 0, 0, 1}, {-1, 0, 0, 0, -1, 0, 0, 0, 1},
    {0, -1, 0, 1, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 1, 0, 0, 0, 1},  {0, 0, -1, -1, 0, 0, 0, 1, 0}};

template <typename TS>
__global__ __launch_bounds__(LB) void latlon_in_prepare_kernel(const TS* __restrict__ src, double* __restrict__ work,
                                                               int nlat, int nlon, double lat0, double dlat,
                                                               double lon0, double dlon, int poles, int has_h,
                                                               int has_wind, int nq) {
  __shared__ double sv[3][PCH];
  __shared__ double mean[3];
  const int j = blockIdx.x, tid = threadIdx.x;
  const size_t K = (size_t)nlat * nlon, r0 = (size_t)j * nlon;
  // scalars: h first, the tracers after the wind
  if (has_h)
    for (int i = tid; i < nlon; i += LB) work[r0 + i] = (double)src[r0 + i];
  const int cin_q = has_h + 2 * has_wind, cw_q = has_h + 3 * has_wind;
  for (int k = 0; k < nq; ++k)
    for (int i = tid; i < nlon; i += LB) work[(size_t)(cw_q + k) * K + r0 + i] = (double)src[(size_t)(cin_q + k) * K + r0 + i];
  if (!has_wind) return;
  const TS* u = src + (size_t)has_h * K + r0;
  const TS* v = u + K;
  double* V = work + (size_t)has_h * K + r0;
  double sp, cp;
  sincos(lat0 + (double)j * dlat, &sp, &cp);
  const bool pole = poles && (j == 0 || j == nlat - 1);
  double acc = 0.0;
  for (int c0 = 0; c0 < nlon; c0 += PCH) {      // one pass unless the row is a pole row
    const int cn = min(PCH, nlon - c0);
    for (int i = c0 + tid; i < (pole ? c0 + cn : nlon); i += LB) {
      double sl, cl;
      sincos(lon0 + (double)i * dlon, &sl, &cl);
      const double uu = (double)u[i], vv = (double)v[i];
      const double vx = -(uu * sl) - vv * (sp * cl), vy = uu * cl - vv * (sp * sl), vz = vv * cp;
      if (pole) {
        sv[0][i - c0] = vx;
        sv[1][i - c0] = vy;
        sv[2][i - c0] = vz;
      } else {
        V[i] = vx;
        V[K + i] = vy;
        V[2 * K + i] = vz;
      }
    }
    if (!pole) return;
    __syncthreads();
    if (tid < 3)
      for (int i = 0; i < cn; ++i) acc = acc + sv[tid][i];
    __syncthreads();
  }
  if (tid < 3) mean[tid] = acc / (double)nlon;
  __syncthreads();
  for (int i = tid; i < nlon; i += LB) {
    V[i] = mean[0];
    V[K + i] = mean[1];
    V[2 * K + i] = mean[2];
  }
}

template <int ORDER>
__device__ __forceinline__ void tap_weights(double t, double* w) {
  if (ORDER == 1) {
    w[0] = 1.0 - t;
    w[1] = t;
  } else {
    const double tm = t - 1.0, tp = t + 1.0, t2 = t - 2.0;
    w[0] = -(t * tm * t2) / 6.0;
    w[1] = (tp * tm * t2) / 2.0;
    w[2] = -(tp * t * t2) / 2.0;
    w[3] = (tp * t * tm) / 6.0;
  }
}

template <int Q>
__device__ __forceinline__ void gauss(int a, double* g, double* w) {
  if (Q == 1) {
    *g = 0.0;
    *w = 2.0;
  } else if (Q == 2) {
    *g = a ? 0.5773502691896257 : -0.5773502691896257;
    *w = 1.0;
  } else {
    const double n = (a == 0 || a == 3) ? 0.8611363115940526 : 0.3399810435848563;
    *g = a < 2 ? -n : n;
    *w = (a == 0 || a == 3) ? 0.3478548451374538 : 0.6521451548625461;
  }
}

// unit vector p of the equiangular point ((2 I + 1 - N) + ga, (2 J + 1 - N) + gb) dalpha / 2 of a panel
// and the area density of the map there
__device__ __forceinline__ double gnomonic(const int* fr, int N, int I, int J, double ga, double gb, double* p) {
  const double half = 0.25 * M_PI / (double)N;
  const double X = tan(((double)(2 * I + 1 - N) + ga) * half), Y = tan(((double)(2 * J + 1 - N) + gb) * half);
  const double r2 = 1.0 + X * X + Y * Y, r = sqrt(r2);
#pragma unroll
  for (int c = 0; c < 3; ++c) p[c] = ((double)fr[c] + X * (double)fr[3 + c] + Y * (double)fr[6 + c]) / r;
  return ((1.0 + X * X) * (1.0 + Y * Y)) / (r2 * r);
}

// val[k] for a run-time k without indexing the register array (no scratch)
__device__ __forceinline__ double pick(const double* val, int k) {
  double r = val[0];
#pragma unroll
  for (int c = 1; c < MAXC; ++c) r = k == c ? val[c] : r;
  return r;
}

template <typename T, int ORDER, int Q>
__global__ __launch_bounds__(LB) void latlon_in_ingest_kernel(const LatLonInDesc d) {
  constexpr int L = Q * Q, NT = ORDER == 1 ? 2 : 4, FIRST = ORDER == 1 ? 0 : -1;
  constexpr int ROWS = BLK / L;                 // rows of the block this workgroup serves
  const int nb = (d.n + BLK - 1) / BLK;
  const int sub = blockIdx.x % L, blk = blockIdx.x / L;
  const int tile = blk / (nb * nb), by = (blk / nb) % nb, bx = blk % nb;
  const int cell = threadIdx.x / L, lane = threadIdx.x % L;
  const int i = bx * BLK + cell % BLK, j = by * BLK + sub * ROWS + cell / BLK;
  const bool on = i < d.n && j < d.n;
  const int* to = d.tiles + 3 * tile;
  const int* fr = FRAMES[to[0]];
  const int I = to[1] + i, J = to[2] + j;
  const size_t K = (size_t)d.nlat * d.nlon;
  double val[MAXC], wq = 0.0;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) val[c] = 0.0;
  if (on) {
    double ga, gb, wa, wb, p[3];
    gauss<Q>(lane % Q, &ga, &wa);
    gauss<Q>(lane / Q, &gb, &wb);
    wq = (wa * wb) * gnomonic(fr, d.N, I, J, ga, gb, p);
    const double lat = asin(fmin(fmax(p[2], -1.0), 1.0));
    double lon = atan2(p[1], p[0]);
    if (lon < 0.0) lon = lon + 2.0 * M_PI;
    const double x = (lon - d.lon0) / d.dlon, y = (lat - d.lat0) / d.dlat;
    const double fx = floor(x), fy = fmin(fmax(floor(y), -1.0), (double)(d.nlat - 1));
    double wx[NT], wy[NT];
    tap_weights<ORDER>(x - fx, wx);
    tap_weights<ORDER>(y - fy, wy);
    // columns: wrapped, and shifted by nlon / 2 for a row reflected across a pole
    int col[NT], cols[NT], row[NT];
    bool refl[NT];
    const int i0 = (int)fx + FIRST, j0 = (int)fy + FIRST, hl = d.nlon / 2;
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      int c = (i0 + b) % d.nlon;
      c = c < 0 ? c + d.nlon : c;
      col[b] = c;
      cols[b] = c + hl >= d.nlon ? c + hl - d.nlon : c + hl;
      const int r = j0 + b;
      refl[b] = r < 0 || r > d.nlat - 1;
      row[b] = r < 0 ? (d.poles ? -r : -1 - r) : (r > d.nlat - 1 ? (d.poles ? 2 * d.nlat - 2 : 2 * d.nlat - 1) - r : r);
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < d.C) {
        const double* f = d.work + (size_t)c * K;
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < NT; ++a) {
          const double* fr_ = f + (size_t)row[a] * d.nlon;
          double s = wx[0] * fr_[refl[a] ? cols[0] : col[0]];
#pragma unroll
          for (int b = 1; b < NT; ++b) s = s + wx[b] * fr_[refl[a] ? cols[b] : col[b]];
          v = a == 0 ? wy[0] * s : v + wy[a] * s;
        }
        val[c] = v * wq;
      }
    }
  }
  // the cell's lanes: a fixed butterfly, executed by every lane of the wave
#pragma unroll
  for (int m = 1; m < L; m <<= 1) {
    wq = wq + __shfl_xor(wq, m);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < d.C) val[c] = val[c] + __shfl_xor(val[c], m);
  }
  if (!on || lane) return;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) val[c] = val[c] / wq;
  T* q = (T*)d.Q + (size_t)tile * d.pw * d.pw + (size_t)(j + d.mg) * d.pw + (i + d.mg);
  const int c0 = d.has_h;                       // first channel after h
  double h;
  if (d.has_h) {
    h = val[0];
    q[0] = (T)h;
  } else {
    h = (double)q[0];
  }
  if (d.has_wind) {
    double ctr[3];
    gnomonic(fr, d.N, I, J, 0.0, 0.0, ctr);
    const double vx = pick(val, c0), vy = pick(val, c0 + 1), vz = pick(val, c0 + 2);
    const double dn = (vx * ctr[0] + vy * ctr[1]) + vz * ctr[2];
    q[(size_t)d.S] = (T)(h * (vx - dn * ctr[0]));
    q[2 * (size_t)d.S] = (T)(h * (vy - dn * ctr[1]));
    q[3 * (size_t)d.S] = (T)(h * (vz - dn * ctr[2]));
  }
  const int cq = c0 + 3 * d.has_wind;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < d.nq) q[(size_t)d.qfield[k] * d.S] = (T)(h * pick(val, cq + k));
}

template <typename T, int ORDER>
void ingest_q(const LatLonInDesc* d, dim3 grid, hipStream_t s) {
  if (d->quad == 1) hipLaunchKernelGGL((latlon_in_ingest_kernel<T, ORDER, 1>), grid, dim3(LB), 0, s, *d);
  if (d->quad == 2) hipLaunchKernelGGL((latlon_in_ingest_kernel<T, ORDER, 2>), dim3(grid.x * 4), dim3(LB), 0, s, *d);
  if (d->quad == 4) hipLaunchKernelGGL((latlon_in_ingest_kernel<T, ORDER, 4>), dim3(grid.x * 16), dim3(LB), 0, s, *d);
}

template <typename T>
int launch(const LatLonInDesc* d, hipStream_t s) {
  if (d->phases & 1) {
    if (d->src_dtype == 1)
      hipLaunchKernelGGL(latlon_in_prepare_kernel<double>, dim3(d->nlat), dim3(LB), 0, s, (const double*)d->src, d->work,
                         d->nlat, d->nlon, d->lat0, d->dlat, d->lon0, d->dlon, d->poles, d->has_h, d->has_wind, d->nq);
    else
      hipLaunchKernelGGL(latlon_in_prepare_kernel<float>, dim3(d->nlat), dim3(LB), 0, s, (const float*)d->src, d->work,
                         d->nlat, d->nlon, d->lat0, d->dlat, d->lon0, d->dlon, d->poles, d->has_h, d->has_wind, d->nq);
  }
  if (d->phases & 2) {
    const int nb = (d->n + BLK - 1) / BLK;
    const dim3 grid(d->ntile * nb * nb);
    if (d->order == 1) ingest_q<T, 1>(d, grid, s);
    else ingest_q<T, 3>(d, grid, s);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_latlon_in_desc_size(void) { return (int)sizeof(LatLonInDesc); }

// 0 ok; 1 bad pointers / phases / shapes; 2 bad dtype; 3 launch error; 4 bad source grid;
// 5 bad channel description; 6 bad order / quadrature
extern "C" int stsp_latlon_in_launch(int dtype, const LatLonInDesc* d, hipStream_t stream) {
  if (!d || !(d->phases & 3) || (d->phases & ~3) || !d->work) return 1;
  if ((d->phases & 1) && (!d->src || (d->src_dtype != 0 && d->src_dtype != 1))) return 1;
  if (d->nlat < 4 || d->nlon < 8 || (d->nlon & 1) || (long long)d->nlat * d->nlon > (1ll << 28)) return 4;
  if (!(d->dlat > 0.0) || !(d->dlon > 0.0) || !(fabs(d->lon0) <= 2.0 * M_PI) || !(fabs(d->lat0) <= 0.5 * M_PI)) return 4;
  if (d->nq < 0 || d->nq > 4 || (d->has_h & ~1) || (d->has_wind & ~1)) return 5;
  if (d->C != d->has_h + 3 * d->has_wind + d->nq || d->C < 1 || d->C > MAXC) return 5;
  if (d->phases & 2) {
    if (!d->Q || !d->tiles) return 1;
    if (d->ntile <= 0 || d->n <= 0 || d->N < d->n || d->mg < 0 || d->pw != d->n + 2 * d->mg) return 1;
    if (d->S < (long long)d->ntile * d->pw * d->pw) return 1;
    const long long nb = (d->n + BLK - 1) / BLK;
    if ((long long)d->ntile * nb * nb * 16 >= (1ll << 31)) return 1;
    if ((d->order != 1 && d->order != 3) || (d->quad != 1 && d->quad != 2 && d->quad != 4)) return 6;
    for (int k = 0; k < d->nq; ++k)
      if (d->qfield[k] < 4 || d->qfield[k] >= d->F) return 5;
    if (d->F < (d->has_wind ? 4 : 1)) return 5;
  }
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
