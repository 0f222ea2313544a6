// Gradient synthesis on the device: the east and north parts
//   east  = (1 / (R cos phi)) df/dlambda,   north = (1 / R) df/dphi
// of the gradient of up to two band-limited fields
//   f(c) = sum_m sum_(l >= m) P_lm(mu_c) (C_lm cos m lambda_c + S_lm sin m lambda_c)
// at the rank's own cell centres: what the rotational wind k x grad psi and the
// divergent wind grad chi are made of, psi and chi in one launch.  Definitions,
// the packing, the chunk bounds and the PyTorch twin (models/spectra.py::gradient,
// termwise, the oracle) are in models/spectra.py.
//
// Nothing divides by cos phi.  For an order m >= 1 the kernel carries the column
//   Q_lm = P_lm / cos phi,   Q_mm = c_m cos^(m-1) phi,
// which the recurrence of the synthesis produces with the same factors a, b, and
//   d/dlambda:  m Q_lm (S_lm cos m lambda - C_lm sin m lambda)         (times cos phi / cos phi)
//   d/dphi:     dP_lm/dphi = f_lm Q_(l-1)m - l mu Q_lm,  f_lm = sqrt((l^2 - m^2)(2l + 1) / (2l - 1)).
// Q is the only A operand.  Every derivative sits on the coefficients: with K_l one
// of {C, S}_lm the three products of an order are
//   H0 = sum_l Q_lm K_l,   Hl = sum_l Q_lm (l K_l),   Hf = sum_l Q_lm (f_(l+1)m K_(l+1))
// (the shift of f_lm Q_(l-1)m onto the row above; 0 at l = L), and then
//   east  += m (H0^s cos m lambda - H0^c sin m lambda)
//   north += (Hf^c - mu Hl^c) cos m lambda + (Hf^s - mu Hl^s) sin m lambda.
// Six columns a channel, 12 of the 16 columns of one v_mfma_f64_16x16x4 B tile for
// two channels.  Order 0 has dP_l0/dphi = sqrt(l (l+1) / 2) P_l1 = sqrt(l (l+1) / 2)
// cos phi Q_l1: in the rows of order 1 only, columns 12 and 13 hold sqrt(l (l+1) / 2)
// C_l0 of the two channels, and cos phi times that product is all of order 0.  The
// kernel walks the orders 1 .. L and never forms P_l0 / cos phi.
//
// K comes packed (models/spectra.py::pack_gradient): rows (m >= 1, l >= m) in order
// of m then l, row (m-1)(L+1) - (m-1) m / 2 + (l - m); columns 6 ch + {0 .. 5} =
// K^c, K^s, l K^c, l K^s, f K^c_(l+1), f K^s_(l+1); 12 + ch the order-0 rider; 14, 15
// and the columns of an absent channel zeros.
//
//  grad_synth  grid (cell batches) x (order chunks), 128 threads (two waves).  A
//              workgroup owns 128 cells, one per thread, and walks the orders of
//              its chunk in ascending order.  Per order: sincos(m lambda), the
//              start Q_mm (binary powering, m is uniform), then per group of 32
//              degrees 32 steps of the recurrence into LDS and the group's tile
//              [32 x 16] into LDS; after a barrier wave w multiplies its 4 tiles
//              [16 cells x 32 degrees] by the tile with 8 v_mfma_f64_16x16x4 each,
//              the 4 accumulators living across the groups of the order.  After
//              the last group H goes through LDS (row stride 17) to the owning
//              thread, which adds the combinations above to its four register
//              sums (east, north of two channels).  The scale 1 / R is applied once,
//              at the store.  One chunk: into out [C][2][cells] at the cell's
//              index; more: into the workgroup's own record [chunk][2 C][cells].
//  fold        one thread per (plane, cell): the chunks added in ascending order.
//
// No atomics; the summation order is fixed by the launch shape alone, so two calls
// agree bit for bit.  Cells beyond the rank, degrees beyond L, the l = L row of Hf
// and unused columns are zeros by predication or by the packing; only the rank's
// own cells are addressed.  A cell centre on a pole has cos phi = 0: Q_mm = c_1 for
// m = 1 (the powering loop does not run) and 0 above, so only order 1 and its rider
// (times cos phi = 0) contribute there, and the result is the finite vector in the
// frame of lambda = 0.  The LDS layouts and their bank arithmetic are those of
// synth_kernel.hip (Pt rows of 144 doubles, Kt 16, H 17).
#include <cmath>

#include "stsp_kernels.h"

namespace {

constexpr int GB = 128;    // workgroup size = cells per batch
constexpr int GG = 32;     // degrees per group
constexpr int GP = 144;    // Qt row width in doubles (16 mod 32)
constexpr int GH = 17;     // H row width in doubles

typedef double d4 __attribute__((ext_vector_type(4)));

struct alignas(32) Cell4 {
  double mu, cphi, lam, w;
};

__global__ __launch_bounds__(GB) void grad_synth_kernel(const double* __restrict__ K, const int* __restrict__ idx,
                                                        const Cell4* __restrict__ cell, const double* __restrict__ ta,
                                                        const double* __restrict__ tb, const double* __restrict__ tc,
                                                        const int* __restrict__ bounds, double* __restrict__ dst,
                                                        double inv_radius, int C, int cells, int L, int chunks) {
  __shared__ double Qt[GG * GP];
  __shared__ double Kt[GG * 16];
  static_assert(GB * GH <= GG * GP, "H aliases Qt");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = lane >> 4, i16 = lane & 15;
  const int chunk = blockIdx.y;
  const int m_lo = bounds[chunk], m_hi = bounds[chunk + 1];
  const int c = blockIdx.x * GB + tid;
  const bool live = c < cells;
  const int T1 = L + 1;
  double mu = 0.0, cphi = 0.0, lam = 0.0;
  if (live) {
    const Cell4 cl = cell[c];
    mu = cl.mu;
    cphi = cl.cphi;
    lam = cl.lam;
  }
  double east[2] = {0.0, 0.0}, north[2] = {0.0, 0.0};

  for (int m = m_lo; m < m_hi; ++m) {
    const int rows = L + 1 - m;                       // degrees l = m .. L
    const int ngroups = (rows + GG - 1) / GG;
    const double* Km = K + ((size_t)(m - 1) * T1 - (size_t)(m - 1) * m / 2) * 16;
    const double* am = ta + (size_t)m * T1;           // a[m][l], b[m][l]: consecutive along the recurrence
    const double* bm = tb + (size_t)m * T1;
    double sn = 0.0, cn = 0.0, qmm = 0.0;
    if (live) {
      sincos((double)m * lam, &sn, &cn);
      // c_m cos^(m-1) phi
      double pw = 1.0, base = cphi;
      for (int e = m - 1; e > 0; e >>= 1) {
        if (e & 1) pw *= base;
        base *= base;
      }
      qmm = tc[m] * pw;
    }
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    double p1 = 0.0, p2 = 0.0;
    for (int grp = 0; grp < ngroups; ++grp) {
      const int r0 = grp * GG;
      // ---- this cell's column of Q, rows r0 .. r0 + 31 -----------------------------
      if (r0 + GG <= rows) {
        // a whole group: no predicate inside.  Row 0: a[m][m] = b[m][m] = 0 and p1 = p2 = 0,
        // the start replaces it
#pragma unroll 8
        for (int r = 0; r < GG; ++r) {
          const int l = m + r0 + r;
          double p = am[l] * (mu * p1 - bm[l] * p2);
          if (r0 + r == 0) p = qmm;
          p2 = p1;
          p1 = p;
          Qt[r * GP + tid] = p;
        }
      } else {
#pragma unroll 4
        for (int r = 0; r < GG; ++r) {
          const int rr = r0 + r;
          double p = 0.0;
          if (rr < rows) {
            if (rr == 0) {
              p = qmm;
            } else {
              const int l = m + rr;
              p = am[l] * (mu * p1 - bm[l] * p2);
            }
            p2 = p1;
            p1 = p;
          }
          Qt[r * GP + tid] = p;
        }
      }
      // ---- the group's tile: 512 entries, 4 per thread, consecutive in memory ---------
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = tid + GB * k;
        const int rr = r0 + (e >> 4);
        Kt[e] = rr < rows ? Km[(size_t)rr * 16 + (e & 15)] : 0.0;
      }
      __syncthreads();
      // ---- wave wv: its 4 tiles of 16 cells times the tile ------------------------------
#pragma unroll
      for (int kk = 0; kk < GG / 4; ++kk) {
        const double bv = Kt[(4 * kk + q) * 16 + i16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double av = Qt[(4 * kk + q) * GP + 64 * wv + 16 * t + i16];
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    // ---- H [cell][column] to the owning thread (H aliases Qt: every read of Qt is behind
    // the barrier above) ----------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) Qt[(64 * wv + 16 * t + 4 * r + q) * GH + i16] = acc[t][r];
    __syncthreads();
    const double* h = Qt + tid * GH;
    const double dm = (double)m;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const double h0c = h[6 * ch], h0s = h[6 * ch + 1], hlc = h[6 * ch + 2], hls = h[6 * ch + 3];
      const double hfc = h[6 * ch + 4], hfs = h[6 * ch + 5];
      east[ch] += dm * (h0s * cn - h0c * sn);
      north[ch] += (hfc - mu * hlc) * cn + (hfs - mu * hls) * sn;
      if (m == 1) north[ch] += cphi * h[12 + ch];      // all of order 0
    }
    __syncthreads();
  }
  if (live) {
    // one chunk: dst is out [C][2][cells], stored at the cell's index; more: dst is the
    // records [chunk][2 C][cells] in the kernel's own cell order
    const size_t at = chunks == 1 ? (size_t)idx[c] : (size_t)chunk * 2 * C * cells + c;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
      if (ch < C) {
        dst[at + (size_t)(2 * ch) * cells] = east[ch] * inv_radius;
        dst[at + (size_t)(2 * ch + 1) * cells] = north[ch] * inv_radius;
      }
  }
}

__global__ __launch_bounds__(256) void grad_fold_kernel(const double* __restrict__ rec, const int* __restrict__ idx,
                                                        double* __restrict__ out, int planes, int cells, int chunks) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)planes * cells;
  if (t >= total) return;
  const int c = (int)(t % cells);
  const size_t pl = t / cells;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += rec[(size_t)k * total + t];
  out[pl * cells + (size_t)idx[c]] = s;
}

}  // namespace

extern "C" int stsp_grad_synth_desc_size(void) { return (int)sizeof(GradSynthDesc); }

extern "C" int stsp_grad_synth_launch(const GradSynthDesc* d, hipStream_t s) {
  if (!d || !d->K || !d->idx || !d->cell || !d->a || !d->b || !d->c || !d->bounds || !d->bounds_dev || !d->out)
    return 1;
  const int L = d->lmax;
  if (L < 1 || L > 1023 || d->C < 1 || d->C > 2 || d->cells < 1) return 1;
  if (d->k_rows != (long long)L * (L + 1) / 2) return 1;
  if (d->idx_limit != d->cells) return 1;             // the index table addresses [0, cells): unpadded output
  if (!(d->inv_radius > 0.0) || !std::isfinite(d->inv_radius)) return 1;
  if (((uintptr_t)d->cell & 31) || ((uintptr_t)d->idx & 3) || ((uintptr_t)d->bounds_dev & 3)) return 1;
  // chunk bounds: 1 = b[0] < b[1] < ... < b[chunks] = L + 1: every order 1 .. L once, no empty chunk
  if (d->chunks < 1 || d->chunks > L) return 1;
  if (d->bounds[0] != 1 || d->bounds[d->chunks] != L + 1) return 1;
  for (int k = 0; k < d->chunks; ++k)
    if (d->bounds[k + 1] <= d->bounds[k]) return 1;
  const int planes = 2 * d->C;
  if (d->chunks > 1) {
    if (!d->rec || d->rec_elems < (long long)d->chunks * planes * d->cells) return 1;
  }
  const long long nbatch = ((long long)d->cells + GB - 1) / GB;
  if (nbatch > 0x7fffffffLL || d->chunks > 65535) return 1;
  hipLaunchKernelGGL(grad_synth_kernel, dim3((unsigned)nbatch, d->chunks), dim3(GB), 0, s, d->K, d->idx,
                     (const Cell4*)d->cell, d->a, d->b, d->c, d->bounds_dev, d->chunks == 1 ? d->out : d->rec,
                     d->inv_radius, d->C, d->cells, L, d->chunks);
  if (d->chunks > 1) {
    const size_t total = (size_t)planes * d->cells;
    hipLaunchKernelGGL(grad_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d->rec, d->idx,
                       d->out, planes, d->cells, d->chunks);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
