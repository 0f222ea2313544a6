// Spherical-harmonic synthesis on the device: the band-limited field
//   f_ch(c) = sum_m sum_(l >= m) P_lm(mu_c) (C_lm cos m lambda_c + S_lm sin m lambda_c)
// of up to 8 channels at once at the rank's own cell centres; the inverse of
// spectra_kernel.hip.  Definitions, the coefficient packing, the chunk bounds
// and the PyTorch twin (models/spectra.py::synthesise, the oracle) are in
// models/spectra.py.
//
// For one order m the work is a tall product  H[c, j] = sum_l P_lm(mu_c) K[l, j]
// with the 2 C <= 16 columns K[l, 2 ch + s] = {C, S}_lm of channel ch, followed by
//   f_ch(c) += H[c, 2 ch] cos m lambda_c + H[c, 2 ch + 1] sin m lambda_c.
// The rows of P are generated on the fly by the column recurrence, as in the
// analysis; nothing of the basis is ever stored in memory.  The recurrence walks
// l at fixed m, so its factors come transposed, a[m][l] and b[m][l] (copies that
// ops/spectra.py makes of the rank's tables): the steps of a whole group read
// consecutive doubles, which the compiler fetches 8 at a time into scalar
// registers; read as [l][m] every step touched a cache line of its own, and the
// launch at C720, lmax 255 took 198 ms instead of 124 (profiles/synthesis).
//
// K comes packed (models/spectra.py::pack_coeffs): rows (m, l >= m) in order of
// m then l, row m (L+1) - m (m-1) / 2 + (l - m), 16 columns, zeros beyond 2 C and
// in the sine column of m = 0.  The packing reads the lower triangle only, so
// what the caller's array holds at m > l or in S_l0 never reaches the kernel.
//
//  synth    grid (cell batches) x (order chunks), 128 threads (two waves).  A
//           workgroup owns 128 cells, one per thread (one 32-byte load of mu,
//           cos phi, lambda, w), and walks the orders m of its chunk in ascending
//           order.  Per order: sincos(m lambda), the sectoral start
//           P_mm = c_m cos^m phi (binary powering, m is uniform), and then per
//           group of 32 degrees 32 steps of the recurrence into LDS and the
//           group's K tile [32 x 16] into LDS; after a barrier wave w multiplies
//           its 4 tiles [16 cells x 32 degrees] by the K tile with 8
//           v_mfma_f64_16x16x4 each (A = cells x degrees, B = degrees x columns),
//           the 4 accumulators living across the groups of the order.  After the
//           last group H goes through LDS to the owning thread, which adds the
//           cos / sin combination to its 8 per-channel register accumulators.
//           One chunk: the thread stores its C values into the field.  More: it
//           stores them into the workgroup's own record [chunk][C][cells].
//  fold     one thread per (channel, cell): the chunks' records added in ascending
//           chunk order.
//
// No atomics; the summation order is fixed by the launch shape alone (chunk
// bounds, degree order inside the matrix core's 16 x 16 x 4 step), so two calls
// agree bit for bit.  Cells beyond the rank, degrees beyond L and columns beyond
// 2 C are zeros by predication; nothing is padded and only the rank's own cells
// are addressed.  Nothing divides by cos phi: a cell centre on a pole has
// cos phi = 0, so P_mm = 0 for m > 0 and 1 for m = 0 (the powering loop does not
// run), and the column recurrence goes on from there.
//
// LDS (64 banks of 4 bytes; ds_read_b64 is served in two groups of 32 lanes,
// ds_write_b64 in four groups of 16):
//   Pt [32 degrees][144]  a thread writes its cell's column: 16 consecutive lanes,
//                         16 consecutive doubles.  The A operand of lane (q = lane
//                         >> 4, i = lane & 15) is Pt[4 kk + q][16 t + i]: within 32
//                         lanes q takes two values, and 144 = 16 mod 32 puts the
//                         second row 16 doubles on, so the 32 reads cover 32
//                         distinct doubles = all 64 banks once.
//   Kt [32 degrees][16]   the B operand Kt[4 kk + q][i] is 32 consecutive doubles.
//   H  [128 cells][17]    aliases Pt after the order's last product: written 16
//                         consecutive doubles per 16 lanes, read by the owning
//                         thread at stride 17 doubles = 34 dwords, 32 distinct even
//                         banks.
#include "stsp_kernels.h"

namespace {

constexpr int YB = 128;    // workgroup size = cells per batch
constexpr int YG = 32;     // degrees per group
constexpr int YP = 144;    // Pt row width in doubles (16 mod 32)
constexpr int YH = 17;     // H row width in doubles

typedef double d4 __attribute__((ext_vector_type(4)));

struct alignas(32) Cell4 {
  double mu, cphi, lam, w;
};

__global__ __launch_bounds__(YB) void synth_kernel(const double* __restrict__ K, const int* __restrict__ idx,
                                                   const Cell4* __restrict__ cell, const double* __restrict__ ta,
                                                   const double* __restrict__ tb, const double* __restrict__ tc,
                                                   const int* __restrict__ bounds, double* __restrict__ dst, int C,
                                                   int cells, int L, int chunks) {
  __shared__ double Pt[YG * YP];
  __shared__ double Kt[YG * 16];
  static_assert(YB * YH <= YG * YP, "H aliases Pt");
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int q = lane >> 4, i16 = lane & 15;
  const int chunk = blockIdx.y;
  const int m_lo = bounds[chunk], m_hi = bounds[chunk + 1];
  const int c = blockIdx.x * YB + tid;
  const bool live = c < cells;
  const int T1 = L + 1;
  double mu = 0.0, cphi = 0.0, lam = 0.0;
  if (live) {
    const Cell4 cl = cell[c];
    mu = cl.mu;
    cphi = cl.cphi;
    lam = cl.lam;
  }
  double f[8];
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) f[ch] = 0.0;

  for (int m = m_lo; m < m_hi; ++m) {
    const int rows = L + 1 - m;                       // degrees l = m .. L
    const int ngroups = (rows + YG - 1) / YG;
    const double* Km = K + ((size_t)m * T1 - (size_t)m * (m - 1) / 2) * 16;
    const double* am = ta + (size_t)m * T1;           // a[m][l], b[m][l]: consecutive along the recurrence
    const double* bm = tb + (size_t)m * T1;
    double sn = 0.0, cn = 0.0, pmm = 0.0;
    if (live) {
      sincos((double)m * lam, &sn, &cn);
      // c_m cos^m phi
      double pw = 1.0, base = cphi;
      for (int e = m; e > 0; e >>= 1) {
        if (e & 1) pw *= base;
        base *= base;
      }
      pmm = tc[m] * pw;
    }
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    double p1 = 0.0, p2 = 0.0;
    for (int grp = 0; grp < ngroups; ++grp) {
      const int r0 = grp * YG;
      // ---- this cell's column, rows r0 .. r0 + 31 ----------------------------------
      if (r0 + YG <= rows) {
        // a whole group: no predicate inside, so that the factors of consecutive steps are
        // fetched together.  Row 0: a[m][m] = b[m][m] = 0 and p1 = p2 = 0, the start replaces it
#pragma unroll 8
        for (int r = 0; r < YG; ++r) {
          const int l = m + r0 + r;
          double p = am[l] * (mu * p1 - bm[l] * p2);
          if (r0 + r == 0) p = pmm;
          p2 = p1;
          p1 = p;
          Pt[r * YP + tid] = p;
        }
      } else {
#pragma unroll 4
        for (int r = 0; r < YG; ++r) {
          const int rr = r0 + r;
          double p = 0.0;
          if (rr < rows) {
            if (rr == 0) {
              p = pmm;
            } else {
              const int l = m + rr;
              p = am[l] * (mu * p1 - bm[l] * p2);
            }
            p2 = p1;
            p1 = p;
          }
          Pt[r * YP + tid] = p;
        }
      }
      // ---- the group's K tile: 512 entries, 4 per thread, consecutive in memory ------
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int e = tid + YB * k;
        const int rr = r0 + (e >> 4);
        Kt[e] = rr < rows ? Km[(size_t)rr * 16 + (e & 15)] : 0.0;
      }
      __syncthreads();
      // ---- wave wv: its 4 tiles of 16 cells times the K tile ---------------------------
#pragma unroll
      for (int kk = 0; kk < YG / 4; ++kk) {
        const double bv = Kt[(4 * kk + q) * 16 + i16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double av = Pt[(4 * kk + q) * YP + 64 * wv + 16 * t + i16];
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    // ---- H [cell][column] to the owning thread (H aliases Pt: every read of Pt is behind
    // the barrier above) ----------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) Pt[(64 * wv + 16 * t + 4 * r + q) * YH + i16] = acc[t][r];
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < C) f[ch] += Pt[tid * YH + 2 * ch] * cn + Pt[tid * YH + 2 * ch + 1] * sn;
    __syncthreads();
  }
  if (live) {
    // one chunk: dst is the field [C][cells], stored at the cell's index; more: dst is
    // the records [chunk][C][cells] in the kernel's own cell order
    const size_t at = chunks == 1 ? (size_t)idx[c] : (size_t)chunk * C * cells + c;
#pragma unroll
    for (int ch = 0; ch < 8; ++ch)
      if (ch < C) dst[at + (size_t)ch * cells] = f[ch];
  }
}

__global__ __launch_bounds__(256) void synth_fold_kernel(const double* __restrict__ rec, const int* __restrict__ idx,
                                                         double* __restrict__ out, int C, int cells, int chunks) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)C * cells;
  if (t >= total) return;
  const int c = (int)(t % cells);
  const size_t ch = t / cells;
  double s = 0.0;
  for (int k = 0; k < chunks; ++k) s += rec[(size_t)k * total + t];
  out[ch * cells + (size_t)idx[c]] = s;
}

}  // namespace

extern "C" int stsp_synth_desc_size(void) { return (int)sizeof(SynthDesc); }

extern "C" int stsp_synth_launch(const SynthDesc* d, hipStream_t s) {
  if (!d || !d->K || !d->idx || !d->cell || !d->a || !d->b || !d->c || !d->bounds || !d->bounds_dev || !d->out)
    return 1;
  const int L = d->lmax;
  if (L < 0 || L > 1023 || d->C < 1 || d->C > 8 || d->cells < 1) return 1;
  if (d->k_rows != (long long)(L + 1) * (L + 2) / 2) return 1;
  if (d->idx_limit != d->cells) return 1;             // the index table addresses [0, cells): unpadded output
  if (((uintptr_t)d->cell & 31) || ((uintptr_t)d->idx & 3) || ((uintptr_t)d->bounds_dev & 3)) return 1;
  // chunk bounds: 0 = b[0] < b[1] < ... < b[chunks] = L + 1: every order once, no empty chunk
  if (d->chunks < 1 || d->chunks > L + 1) return 1;
  if (d->bounds[0] != 0 || d->bounds[d->chunks] != L + 1) return 1;
  for (int k = 0; k < d->chunks; ++k)
    if (d->bounds[k + 1] <= d->bounds[k]) return 1;
  if (d->chunks > 1) {
    if (!d->rec || d->rec_elems < (long long)d->chunks * d->C * d->cells) return 1;
  }
  const long long nbatch = ((long long)d->cells + YB - 1) / YB;
  if (nbatch > 0x7fffffffLL || d->chunks > 65535) return 1;
  hipLaunchKernelGGL(synth_kernel, dim3((unsigned)nbatch, d->chunks), dim3(YB), 0, s, d->K, d->idx,
                     (const Cell4*)d->cell, d->a, d->b, d->c, d->bounds_dev, d->chunks == 1 ? d->out : d->rec, d->C,
                     d->cells, L, d->chunks);
  if (d->chunks > 1) {
    const size_t total = (size_t)d->C * d->cells;
    hipLaunchKernelGGL(synth_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d->rec, d->idx,
                       d->out, d->C, d->cells, d->chunks);
  }
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
