// Spherical-harmonic analysis of cell fields on the device: the coefficients
//   C_lm = sum_c w_c f_c P_lm(mu_c) cos m lambda_c,   S_lm likewise with sin
// of up to 8 channels at once.  Definitions, host tables and the PyTorch twin
// are in models/spectra.py.
//
// For one order m the work is a tall product  out[l, j] = sum_c P_lm(mu_c) G[c, j]
// with the 2 C <= 16 columns G[c, 2 ch + s] = w_c f_c {cos, sin}(m lambda_c).
// The rows of P are generated on the fly by the column recurrence; nothing of
// the basis is ever stored in memory.
//
// Two ordinary launches on the caller's stream, nothing persistent, no atomics:
//
//  analyse  grid (m = 0 .. L) x (cell slabs), 128 threads (two waves).  A
//           workgroup streams its slab in batches of 128 cells.  Per batch
//           every thread owns a cell: one 32-byte load of (mu, cos phi, lambda,
//           w), one index, the C values (converted to double at the load),
//           sincos(m lambda), the 16 products into LDS, and the sectoral start
//           P_mm = c_m cos^m phi (binary powering, m is uniform).  Then, per
//           group of 32 degrees, the thread runs 32 steps of the recurrence
//           for its cell into LDS (two 16-row tiles); after a barrier wave w
//           multiplies tile w [16 x 128 cells] by G [128 x 16] with 32
//           v_mfma_f64_16x16x4 over the cells in ascending order.  The 16 x 16
//           result is added to the workgroup's own partial record
//           [slab][m][l - m][16] in memory (the lane that wrote an entry is
//           the one that reads it back in the next batch; the first batch
//           starts from zero), so no accumulator has to live across groups.
//           Cells beyond the slab or the rank, rows beyond L and columns beyond
//           2 C are zeros by predication; the state is never padded.
//  fold     one thread per (m, l, column): the slabs' partials added in
//           ascending slab order, written to out [C][2][L+1][L+1] at [l][m]
//           (the caller zero-fills the rest; S_l0 is written as +0).
//
// The coefficient (0, 0), the area mean, is summed apart and error-free.  It is
// the one coefficient whose terms are the products w f themselves (P_00 = 1,
// cos 0 = 1), and for a field whose mean vanishes (vorticity; anything with the
// symmetry of a wavenumber-4 wave) a plain sum leaves only the rounding residue
// of its own summation order.  Every thread of an order-0 workgroup keeps a
// (hi, lo) pair per channel (two-sum: hi + lo is the exact sum of the hi parts,
// the errors collect in lo), the workgroup and then the fold add the pairs in
// a fixed order, and hi + lo is stored: the sum of the products to an ulp,
// whatever the layout or the slab count.  The twin does the same.
//
// The summation order is fixed by the launch shape alone (slab bounds, batch
// order, the matrix core's own order inside a 16 x 16 x 4 step), so two calls
// on one state agree bit for bit.  The source layout (padded state or
// unpadded tiles) is a matter of which index table is passed; only interior
// cells are ever addressed.
//
// LDS rows are 17 doubles wide: the per-cell writes (stride 34 dwords) then hit
// 32 distinct even banks, and the operand reads (16 consecutive doubles of 4
// cells) stay within a two-way conflict.
#include "stsp_kernels.h"

namespace {

constexpr int SB = 128;    // workgroup size = cells per batch
constexpr int SG = 32;     // degrees per group (two 16-row tiles, one per wave)
constexpr int SW = 17;     // LDS row width in doubles

typedef double d4 __attribute__((ext_vector_type(4)));

// error-free accumulation: (hi, lo) += x with hi + lo carrying the exact sum of the
// hi parts (Knuth's two-sum) and lo their rounding errors
__device__ __forceinline__ void dd_add(double& hi, double& lo, double x) {
  const double s = hi + x;
  const double bb = s - hi;
  lo += (hi - (s - bb)) + (x - bb);
  hi = s;
}

struct alignas(32) Cell4 {
  double mu, cphi, lam, w;
};

template <typename T>
__global__ __launch_bounds__(SB) void spectra_analyse_kernel(const T* __restrict__ Q, const int* __restrict__ idx,
                                                             const Cell4* __restrict__ cell,
                                                             const double* __restrict__ ta,
                                                             const double* __restrict__ tb,
                                                             const double* __restrict__ tc,
                                                             double* __restrict__ partial, size_t cs, int C,
                                                             int cells, int slab_cells, int L, int RP) {
  __shared__ double Pt[2][SB][SW];
  __shared__ double G[SB][SW];
  const int m = blockIdx.x, slab = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int c_lo = slab * slab_cells;
  const int c_hi = min(cells, c_lo + slab_cells);
  const int rows = L + 1 - m;                       // degrees l = m .. L
  const int ngroups = (rows + SG - 1) / SG;
  const double cm = tc[m];
  double* prec = partial + ((size_t)slab * (L + 1) + m) * (size_t)RP * 16;
  const int T1 = L + 1;
  double mh[8], ml[8];                              // order 0: the area means, error-free
#pragma unroll
  for (int ch = 0; ch < 8; ++ch) mh[ch] = ml[ch] = 0.0;

  for (int c0 = c_lo, batch = 0; c0 < c_hi; c0 += SB, ++batch) {
    const int c = c0 + tid;
    const bool live = c < c_hi;
    double mu = 0.0, pmm = 0.0;
    {
      double g[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) g[j] = 0.0;
      if (live) {
        const Cell4 cl = cell[c];
        const size_t src = (size_t)idx[c];
        double sn, cn;
        sincos((double)m * cl.lam, &sn, &cn);
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) {
          if (ch < C) {
            const double wf = (double)Q[(size_t)ch * cs + src] * cl.w;
            g[2 * ch] = wf * cn;
            g[2 * ch + 1] = wf * sn;
            if (m == 0) dd_add(mh[ch], ml[ch], wf);
          }
        }
        mu = cl.mu;
        // c_m cos^m phi
        double pw = 1.0, base = cl.cphi;
        for (int e = m; e > 0; e >>= 1) {
          if (e & 1) pw *= base;
          base *= base;
        }
        pmm = cm * pw;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) G[tid][j] = g[j];
    }
    double p1 = 0.0, p2 = 0.0;
    for (int grp = 0; grp < ngroups; ++grp) {
      const int r0 = grp * SG;
      // ---- this cell's column, rows r0 .. r0 + 31 ----------------------------------
#pragma unroll 4
      for (int r = 0; r < SG; ++r) {
        const int rr = r0 + r;
        double p = 0.0;
        if (rr < rows) {
          if (rr == 0) {
            p = pmm;
          } else {
            const int l = m + rr;
            p = ta[(size_t)l * T1 + m] * (mu * p1 - tb[(size_t)l * T1 + m] * p2);
          }
          p2 = p1;
          p1 = p;
        }
        Pt[r >> 4][tid][r & 15] = p;
      }
      __syncthreads();
      // ---- wave wv: tile wv of the group times G -------------------------------------
      const int t0 = r0 + 16 * wv;
      if (t0 < rows) {
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        double* dst = prec + (size_t)(t0 + (lane >> 4)) * 16 + (lane & 15);
        if (batch > 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = dst[(size_t)(4 * r) * 16];
        }
#pragma unroll 8
        for (int k = 0; k < SB; k += 4) {
          const double av = Pt[wv][k + (lane >> 4)][lane & 15];
          const double bv = G[k + (lane >> 4)][lane & 15];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(size_t)(4 * r) * 16] = acc[r];
      }
      __syncthreads();
    }
  }
  // ---- the area mean (l = m = 0, P = 1, cos = 1: the terms are w f themselves) ----------
  // replaces row 0 of the order-0 record: column 2 ch holds hi, column 2 ch + 1 (the sine
  // column, identically 0 at m = 0) holds lo.  Lane j < 16 of wave 0 is the lane that
  // stored (row 0, column j) above, so its store here follows that one in program order.
  if (m == 0) {
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
      G[tid][2 * ch] = mh[ch];
      G[tid][2 * ch + 1] = ml[ch];
    }
    __syncthreads();
    if (tid < 16) {
      const int ch = tid >> 1;
      double hi = 0.0, lo = 0.0;
      for (int k = 0; k < SB; ++k) {
        dd_add(hi, lo, G[k][2 * ch]);
        lo += G[k][2 * ch + 1];
      }
      prec[tid] = (tid & 1) ? lo : hi;
    }
  }
}

__global__ __launch_bounds__(256) void spectra_fold_kernel(const double* __restrict__ partial, double* __restrict__ out,
                                                           int C, int L, int RP, int slabs) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int T1 = L + 1;
  const size_t total = (size_t)T1 * RP * 16;
  if (t >= total) return;
  const int j = (int)(t & 15);
  const int r = (int)((t >> 4) % RP);
  const int m = (int)((t >> 4) / RP);
  const int l = m + r;
  if (l > L || j >= 2 * C) return;
  const size_t stride = (size_t)T1 * RP * 16;
  double s = 0.0;
  if (m == 0 && r == 0 && !(j & 1)) {               // the area mean: (hi, lo) pairs, error-free
    double lo = 0.0;
    for (int k = 0; k < slabs; ++k) {
      dd_add(s, lo, partial[(size_t)k * stride + t]);
      lo += partial[(size_t)k * stride + t + 1];
    }
    s += lo;
  } else {
    for (int k = 0; k < slabs; ++k) s += partial[(size_t)k * stride + t];
  }
  if (m == 0 && (j & 1)) s = 0.0;
  out[(((size_t)(j >> 1) * 2 + (j & 1)) * T1 + l) * T1 + m] = s;
}

template <typename T>
int launch(const SpectraDesc* d, hipStream_t s) {
  const int L = d->lmax;
  hipLaunchKernelGGL(spectra_analyse_kernel<T>, dim3(L + 1, d->slabs), dim3(SB), 0, s, (const T*)d->Q, d->idx,
                     (const Cell4*)d->cell, d->a, d->b, d->c, d->partial, (size_t)d->cs, d->C, d->cells,
                     d->slab_cells, L, d->RP);
  const size_t total = (size_t)(L + 1) * d->RP * 16;
  hipLaunchKernelGGL(spectra_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d->partial, d->out,
                     d->C, L, d->RP, d->slabs);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_spectra_desc_size(void) { return (int)sizeof(SpectraDesc); }

extern "C" int stsp_spectra_launch(int dtype, const SpectraDesc* d, hipStream_t stream) {
  if (!d || !d->Q || !d->idx || !d->cell || !d->a || !d->b || !d->c || !d->partial || !d->out) return 1;
  if (d->lmax < 0 || d->lmax > 1023 || d->C < 1 || d->C > 8 || d->cells < 1 || d->cs < 1) return 1;
  if (d->slabs < 1 || d->slabs > 65535 || d->slab_cells < 1 || d->slab_cells % SB) return 1;
  if ((long long)d->slabs * d->slab_cells < d->cells) return 1;
  if ((long long)(d->slabs - 1) * d->slab_cells >= d->cells) return 1;    // no empty slab: every record is written
  if (d->RP < d->lmax + 1 || d->RP % SG) return 1;
  if (((uintptr_t)d->cell & 31) || ((uintptr_t)d->idx & 3)) return 1;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
