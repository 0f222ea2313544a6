// Local ensemble transform Kalman filter (Hunt, Kostelich & Szunyogh 2007) on a
// batched state [M][F][S] (padded layout; ops/letkf.py; definitions and the
// PyTorch twin: models/letkf.py).  Everything is float64; a float32 state is
// converted at load and rounded once at store.
//
//  prep      one thread per observation k: ybar = ((Y_0k + Y_1k) + ...) / M,
//            Yp[k][m] = Y_mk - ybar (obs-major, M padded with zeros to MP = 16
//            or 32), d_k = y_k - ybar.
//  analysis  one workgroup per 8 x 8 cell block of a tile (ragged at the tile
//            end).  The block's cells are dealt to its waves, one cell per wave
//            at a time ("round").  In every round the workgroup scans the K
//            observations NT at a time, keeps those within 2 Lc + (block radius)
//            of the block's centre by a wave ballot and prefix count (ascending
//            observation order, no atomics) and stages CH = 64 kept rows of Yp
//            in LDS at a time, shared by the waves.  Per chunk a wave
//              - forms its cell's exact weights w_ik = g(s_ik / Lc) / sigma_k^2,
//                one observation per lane (0 where the observation does not
//                apply, so the superset does not enter the result);
//              - accumulates A_i += Yp diag(w) Yp^T with v_mfma_f64_16x16x4
//                (contraction over observations, four per instruction; one tile
//                at MP = 16, the three distinct tiles of the symmetric 2 x 2
//                tile matrix at MP = 32), and the right-hand side Yp (w * d) as
//                column 0 of one more tile per tile row.
//            Then, in the wave, with A and V in LDS: cyclic two-sided Jacobi
//            (round-robin pairs, the disjoint rotations of a step applied by
//            all lanes: rows, then columns of A and V).  A pair is rotated
//            while |a_pq| > 1e-15 sqrt(a_pp a_qq); the first sweep that
//            rotates nothing ends the iteration, and the sweep cap sets the
//            error word.  T = wbar 1^T + V sqrt((M-1)/Lam) V^T
//            replaces A, and every field of the cell is read from the M
//            members (stride member_stride), transformed and written back to
//            the same slots: Xa[m] = xbar + sum_n (X[n] - xbar) T[n][m].
//
// A and V of a wave take 2 * MP * (MP + 1) doubles: four waves per workgroup at
// MP = 16 (256 threads), two at MP = 32 (128 threads), so that the workgroup
// stays inside 64 KiB of LDS with the staged chunk.  Nothing is kept in global
// scratch per cell.  Two runs give the same bits: every sum has a fixed order.
// Plain C++ and vector loads / stores only.
#include "stsp_kernels.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int LB = 8;            // block edge (cells)
constexpr int LC = LB * LB;      // cells of a block
constexpr int CH = 64;           // staged observations (one per lane)
constexpr int SWEEP_CAP = 30;
constexpr double ROT_EPS = 1e-15;    // relative size of an off-diagonal entry that is still rotated

struct KArgs {
  void* Q;
  const double* Yp;
  const double* d;
  const double* p;
  const double* sigma;
  const double* centers;
  int* nobs;
  int* err;
  long long member_stride;
  int M, F, K, ntile, n, S, mg, pw, nb, localised;
  double radius, Lc, cdiag;
};

__device__ __forceinline__ void wsync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// angle between the unit vectors a and b: atan2(|a x b|, a . b)
// (no contraction here and in gaspari_cohn: the weights round as the twin's do, operation by
// operation; the polynomial cancels for r > 1 and a fused evaluation would differ by ~1e-15)
__device__ __forceinline__ double angle(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double dt = (ax * bx + ay * by) + az * bz;
  return atan2(sqrt((cx * cx + cy * cy) + cz * cz), dt);
}

// Gaspari-Cohn (1999) fifth-order compactly supported correlation
__device__ __forceinline__ double gaspari_cohn(double r) {
#pragma clang fp contract(off)
  if (r >= 2.0) return 0.0;
  double g;
  if (r <= 1.0) g = r * r * (r * (r * (-0.25 * r + 0.5) + 0.625) - 5.0 / 3.0) + 1.0;
  else g = r * (r * (r * (r * (r / 12.0 - 0.5) + 0.625) + 5.0 / 3.0) - 5.0) + 4.0 - 2.0 / (3.0 * r);
  return g > 0.0 ? g : 0.0;
}

__global__ __launch_bounds__(256) void letkf_prep_kernel(const double* __restrict__ Y, const double* __restrict__ yv,
                                                         double* __restrict__ Yp, double* __restrict__ d, int M, int MP,
                                                         int K) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  double s = Y[k];
  for (int m = 1; m < M; ++m) s = s + Y[(size_t)m * K + k];
  const double yb = s / (double)M;
  for (int m = 0; m < MP; ++m) Yp[(size_t)k * MP + m] = m < M ? Y[(size_t)m * K + k] - yb : 0.0;
  d[k] = yv[k] - yb;
}

template <typename T, int MP, int NW>
__global__ __launch_bounds__(NW * 64) void letkf_analysis_kernel(const KArgs a) {
  constexpr int NT = NW * 64, LD = MP + 1, NTL = MP / 16;
  __shared__ double s_A[NW][MP * LD];
  __shared__ double s_V[NW][MP * LD];
  __shared__ double s_yp[CH][MP];
  __shared__ double s_p[CH][3];
  __shared__ double s_sig[CH];
  __shared__ double s_d[CH];
  __shared__ double s_w[NW][CH];
  __shared__ double s_wd[NW][CH];
  __shared__ double s_c[LC][3];
  __shared__ double s_ang[LC];
  __shared__ double s_bc[4];          // block centre, keep limit (radians)
  __shared__ double s_rhs[NW][MP];
  __shared__ double s_lam[NW][MP];    // eigenvalues, then sqrt((M-1)/lam)
  __shared__ double s_z[NW][MP];
  __shared__ double s_wb[NW][MP];
  __shared__ double s_x[NW][MP];
  __shared__ double s_xp[NW][MP];
  __shared__ double s_cs[NW][MP];     // (c, s) of the step's pairs
  __shared__ int s_pq[NW][MP];        // (p, q) of the step's pairs
  __shared__ int s_list[CH + NT];
  __shared__ int s_wc[NW];
  __shared__ int s_nmax[NW];

  int blk = blockIdx.x;
  const int xb = blk % a.nb;
  blk /= a.nb;
  const int yb = blk % a.nb;
  const int t = blk / a.nb;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = a.M, K = a.K;
  const int Me = (M + 1) & ~1;        // Jacobi size: M rounded up to even (<= MP)

  // ---- the block's cell centres, its centre and the keep limit -----------------------
  if (tid < LC) {
    const int x = xb * LB + (tid & (LB - 1)), y = yb * LB + (tid >> 3);
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    if (x < a.n && y < a.n) {
      const double* c = a.centers + 3 * (((size_t)t * a.n + y) * a.n + x);
      c0 = c[0];
      c1 = c[1];
      c2 = c[2];
    }
    s_c[tid][0] = c0;
    s_c[tid][1] = c1;
    s_c[tid][2] = c2;
  }
  __syncthreads();
  if (tid == 0) {
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int i = 0; i < LC; ++i) {
      b0 = b0 + s_c[i][0];
      b1 = b1 + s_c[i][1];
      b2 = b2 + s_c[i][2];
    }
    const double nr = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    s_bc[0] = b0 / nr;
    s_bc[1] = b1 / nr;
    s_bc[2] = b2 / nr;
  }
  __syncthreads();
  if (tid < LC) {
    const bool ok = s_c[tid][0] != 0.0 || s_c[tid][1] != 0.0 || s_c[tid][2] != 0.0;
    s_ang[tid] = ok ? angle(s_bc[0], s_bc[1], s_bc[2], s_c[tid][0], s_c[tid][1], s_c[tid][2]) : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    double r = 0.0;
    for (int i = 0; i < LC; ++i) r = s_ang[i] > r ? s_ang[i] : r;
    // triangle inequality on the sphere, with a margin for the rounding of the angles
    s_bc[3] = (2.0 * a.Lc / a.radius + r) * (1.0 + 1e-12) + 1e-12;
  }
  __syncthreads();
  const double bcx = s_bc[0], bcy = s_bc[1], bcz = s_bc[2], lim = s_bc[3];

  double* A = s_A[wv];
  double* V = s_V[wv];
  int wmax = 0;

  for (int rd = 0; rd < LC / NW; ++rd) {
    const int ci = rd * NW + wv;
    const int x = xb * LB + (ci & (LB - 1)), y = yb * LB + (ci >> 3);
    const bool valid = x < a.n && y < a.n;          // uniform in the wave
    const double ccx = s_c[ci][0], ccy = s_c[ci][1], ccz = s_c[ci][2];
    d4 accA[NTL * (NTL + 1) / 2], accR[NTL];
#pragma unroll
    for (int i = 0; i < NTL * (NTL + 1) / 2; ++i) accA[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < NTL; ++i) accR[i] = d4{0.0, 0.0, 0.0, 0.0};
    int nobs = 0;

    // ---- scan, compact, stage, accumulate ---------------------------------------------
    int count = 0;
    for (int base = 0; base < K; base += NT) {
      const int k = base + tid;
      bool keep = false;
      if (k < K) {
        keep = true;
        if (a.localised) keep = angle(bcx, bcy, bcz, a.p[3 * (size_t)k], a.p[3 * (size_t)k + 1], a.p[3 * (size_t)k + 2]) <= lim;
      }
      const unsigned long long bal = __builtin_amdgcn_ballot_w64(keep);
      const int pre = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) s_wc[wv] = __popcll(bal);
      __syncthreads();
      int off = count, tot = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const int c = s_wc[w];
        if (w < wv) off += c;
        tot += c;
      }
      if (keep) s_list[off + pre] = k;
      count += tot;
      __syncthreads();
      const bool last = base + NT >= K;
      while (count >= CH || (last && count > 0)) {
        const int m = count < CH ? count : CH;
        for (int e = tid; e < CH * MP; e += NT) {
          const int j = e / MP, i = e % MP;
          s_yp[j][i] = j < m ? a.Yp[(size_t)s_list[j] * MP + i] : 0.0;
        }
        if (tid < m) {
          const size_t ko = (size_t)s_list[tid];
          s_p[tid][0] = a.p[3 * ko];
          s_p[tid][1] = a.p[3 * ko + 1];
          s_p[tid][2] = a.p[3 * ko + 2];
          s_sig[tid] = a.sigma[ko];
          s_d[tid] = a.d[ko];
        }
        const int rest = count - m;                 // < NT
        const int mv = tid < rest ? s_list[m + tid] : 0;
        __syncthreads();
        if (tid < rest) s_list[tid] = mv;
        if (valid) {
          double w = 0.0, wd = 0.0;
          if (lane < m) {
            double g = 1.0;
            if (a.localised) {
              const double s = a.radius * angle(ccx, ccy, ccz, s_p[lane][0], s_p[lane][1], s_p[lane][2]);
              g = gaspari_cohn(s / a.Lc);
            }
            const double sg = s_sig[lane];
            w = g / (sg * sg);
            wd = w * s_d[lane];
          }
          s_w[wv][lane] = w;
          s_wd[wv][lane] = wd;
          nobs += __popcll(__builtin_amdgcn_ballot_w64(w > 0.0));
          wsync();
          const int col = lane & 15;
          for (int k4 = 0; k4 < m; k4 += 4) {       // rows past m are zero and carry w = 0
            const int kk = k4 + (lane >> 4);
            const double wk = s_w[wv][kk];
            const double br = col == 0 ? s_wd[wv][kk] : 0.0;
            const double y0 = s_yp[kk][col];
            const double a0 = y0 * wk;
            accA[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, y0, accA[0], 0, 0, 0);
            accR[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(y0, br, accR[0], 0, 0, 0);
            if constexpr (NTL == 2) {
              const double y1 = s_yp[kk][16 + col];
              const double a1 = y1 * wk;
              accA[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y0, accA[1], 0, 0, 0);   // rows 16.., columns 0..15
              accA[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, y1, accA[2], 0, 0, 0);
              accR[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(y1, br, accR[1], 0, 0, 0);
            }
          }
        }
        count = rest;
        __syncthreads();
      }
    }
    if (!valid) continue;
    wmax = nobs > wmax ? nobs : wmax;

    // ---- A (lower triangle mirrored, so it is exactly symmetric), rhs, V = I ------------
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * r + (lane >> 4), col = lane & 15;
      if (row >= col) {
        A[row * LD + col] = accA[0][r];
        A[col * LD + row] = accA[0][r];
      }
      if (col == 0) s_rhs[wv][row] = accR[0][r];
      if constexpr (NTL == 2) {
        A[(16 + row) * LD + col] = accA[1][r];
        A[col * LD + 16 + row] = accA[1][r];
        if (row >= col) {
          A[(16 + row) * LD + 16 + col] = accA[2][r];
          A[(16 + col) * LD + 16 + row] = accA[2][r];
        }
        if (col == 0) s_rhs[wv][16 + row] = accR[1][r];
      }
    }
    for (int e = lane; e < MP * MP; e += 64) V[(e / MP) * LD + e % MP] = (e / MP == e % MP) ? 1.0 : 0.0;
    wsync();
    if (lane < MP) A[lane * LD + lane] += a.cdiag;
    wsync();

    // ---- cyclic two-sided Jacobi on the leading Me x Me part ------------------------------
    // a pair is rotated while |a_pq| > ROT_EPS sqrt(a_pp a_qq) (A is positive definite); the
    // iteration ends with the first sweep that rotates nothing
    for (int sw = 0;; ++sw) {
      if (sw >= SWEEP_CAP) {
        if (lane == 0) a.err[0] = 1;
        break;
      }
      unsigned long long rotated = 0ull;
      const int np = Me / 2;
      for (int st = 0; st < Me - 1; ++st) {
        bool rot = false;
        if (lane < np) {
          int p, q;
          if (lane == 0) {
            p = Me - 1;
            q = st;
          } else {
            p = (st + lane) % (Me - 1);
            q = (st - lane + Me - 1) % (Me - 1);
          }
          if (p > q) {
            const int sp = p;
            p = q;
            q = sp;
          }
          const double apq = A[p * LD + q];
          double c = 1.0, s = 0.0;
          const double app = A[p * LD + p], aqq = A[q * LD + q];
          if (fabs(apq) > ROT_EPS * sqrt(app * aqq)) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = tt * c;
            rot = true;
          }
          s_cs[wv][2 * lane] = c;
          s_cs[wv][2 * lane + 1] = s;
          s_pq[wv][2 * lane] = p;
          s_pq[wv][2 * lane + 1] = q;
        }
        rotated |= __builtin_amdgcn_ballot_w64(rot);
        wsync();
        for (int e = lane; e < np * Me; e += 64) {          // rows: A <- J^T A
          const int pr = e / Me, j = e % Me;
          const int p = s_pq[wv][2 * pr], q = s_pq[wv][2 * pr + 1];
          const double c = s_cs[wv][2 * pr], s = s_cs[wv][2 * pr + 1];
          const double ap = A[p * LD + j], aq = A[q * LD + j];
          A[p * LD + j] = c * ap - s * aq;
          A[q * LD + j] = s * ap + c * aq;
        }
        wsync();
        for (int e = lane; e < np * Me; e += 64) {          // columns: A <- A J, V <- V J
          const int pr = e / Me, i = e % Me;
          const int p = s_pq[wv][2 * pr], q = s_pq[wv][2 * pr + 1];
          const double c = s_cs[wv][2 * pr], s = s_cs[wv][2 * pr + 1];
          const double ap = A[i * LD + p], aq = A[i * LD + q];
          A[i * LD + p] = c * ap - s * aq;
          A[i * LD + q] = s * ap + c * aq;
          const double vp = V[i * LD + p], vq = V[i * LD + q];
          V[i * LD + p] = c * vp - s * vq;
          V[i * LD + q] = s * vp + c * vq;
        }
        wsync();
        if (lane < np && s_cs[wv][2 * lane + 1] != 0.0) {   // the annihilated pair is exactly zero
          const int p = s_pq[wv][2 * lane], q = s_pq[wv][2 * lane + 1];
          A[p * LD + q] = 0.0;
          A[q * LD + p] = 0.0;
        }
        wsync();
      }
      if (rotated == 0ull) break;
    }

    // ---- wbar = V Lam^-1 V^T rhs;  T = wbar 1^T + V sqrt((M-1)/Lam) V^T  (into A) ----------
    if (lane < Me) {
      const double lam = A[lane * LD + lane];
      double zz = 0.0;
      for (int nn = 0; nn < Me; ++nn) zz = zz + V[nn * LD + lane] * s_rhs[wv][nn];
      s_z[wv][lane] = zz / lam;
      s_lam[wv][lane] = sqrt((double)(M - 1) / lam);
    }
    wsync();
    if (lane < Me) {
      double wb = 0.0;
      for (int j = 0; j < Me; ++j) wb = wb + V[lane * LD + j] * s_z[wv][j];
      s_wb[wv][lane] = wb;
    }
    wsync();
    for (int e = lane; e < Me * Me; e += 64) {
      const int nn = e / Me, mm = e % Me;
      double acc = 0.0;
      for (int j = 0; j < Me; ++j) acc = acc + (V[nn * LD + j] * s_lam[wv][j]) * V[mm * LD + j];
      A[nn * LD + mm] = s_wb[wv][nn] + acc;
    }
    wsync();

    // ---- the cell's fields, in place --------------------------------------------------------
    const size_t cell = (size_t)((t * a.pw + y + a.mg) * a.pw + x + a.mg);
    for (int f = 0; f < a.F; ++f) {
      T* q = (T*)a.Q + (size_t)f * (size_t)a.S + cell + (size_t)lane * (size_t)a.member_stride;
      if (lane < M) s_x[wv][lane] = (double)q[0];
      wsync();
      double xs = s_x[wv][0];
      for (int nn = 1; nn < M; ++nn) xs = xs + s_x[wv][nn];
      const double xbar = xs / (double)M;
      if (lane < M) s_xp[wv][lane] = s_x[wv][lane] - xbar;
      wsync();
      if (lane < M) {
        double acc = 0.0;
        for (int nn = 0; nn < M; ++nn) acc = acc + s_xp[wv][nn] * A[nn * LD + lane];
        q[0] = (T)(xbar + acc);
      }
      wsync();
    }
  }
  if (lane == 0) s_nmax[wv] = wmax;
  __syncthreads();
  if (tid == 0) {
    int mx = 0;
    for (int w = 0; w < NW; ++w) mx = s_nmax[w] > mx ? s_nmax[w] : mx;
    a.nobs[blockIdx.x] = mx;
  }
}

template <typename T>
int launch(const LetkfDesc* d, hipStream_t s) {
  const int MP = d->Mpad;
  hipLaunchKernelGGL(letkf_prep_kernel, dim3((d->K + 255) / 256), dim3(256), 0, s, d->Y, d->yv, d->Yp, d->d, d->M, MP,
                     d->K);
  if (hipGetLastError() != hipSuccess) return 3;
  KArgs a;
  a.Q = d->Q;
  a.Yp = d->Yp;
  a.d = d->d;
  a.p = d->p;
  a.sigma = d->sigma;
  a.centers = d->centers;
  a.nobs = d->nobs;
  a.err = d->err;
  a.member_stride = d->member_stride;
  a.M = d->M;
  a.F = d->F;
  a.K = d->K;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nb = (d->n + LB - 1) / LB;
  a.localised = d->localised;
  a.radius = d->radius;
  a.Lc = d->localised ? d->Lc : 1.0;
  a.cdiag = (double)(d->M - 1) / d->rho;
  if (MP == 16) hipLaunchKernelGGL((letkf_analysis_kernel<T, 16, 4>), dim3(d->nblocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((letkf_analysis_kernel<T, 32, 2>), dim3(d->nblocks), dim3(128), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_letkf_desc_size(void) { return (int)sizeof(LetkfDesc); }

// 1: a descriptor that does not describe a batched state; 2: unknown dtype; 3: launch error;
// 4: members outside 2 .. 32 (or Mpad not their tile padding); 5: observations outside 1 .. 65535;
// 6: localisation length, radius or inflation out of range
extern "C" int stsp_letkf_launch(int dtype, const LetkfDesc* d, hipStream_t stream) {
  if (!d) return 1;
  if (d->M < STSP_LETKF_MIN_M || d->M > STSP_LETKF_MAX_M || d->Mpad != (d->M <= 16 ? 16 : 32)) return 4;
  if (d->K < 1 || d->K > STSP_LETKF_MAX_K) return 5;
  if (d->ntile <= 0 || d->n <= 0 || d->mg < 0 || d->F < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  if (d->member_stride < (long long)d->F * d->S) return 1;
  const int nb = (d->n + LB - 1) / LB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->Q || !d->Y || !d->yv || !d->Yp || !d->d || !d->p || !d->sigma || !d->centers || !d->nobs || !d->err) return 1;
  if (!(d->radius > 0.0) || !(d->rho >= 1.0) || (d->localised && !(d->Lc > 0.0))) return 6;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
