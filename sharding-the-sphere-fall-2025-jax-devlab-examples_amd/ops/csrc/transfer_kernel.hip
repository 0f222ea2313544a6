// Grid transfer on the device: the rank's padded state on C_N from a global
// unpadded state on C_Ns, N = r Ns (refine) or Ns = r N (coarsen), r in 2, 4, 8.
// The definitions and the float64 twin are models/transfer.py; a "fold" below is
// the twin's: a left-to-right sum over a parent's children, rows then columns.
//
// One ordinary launch on the caller's stream, no atomics, nothing persistent.
//
//  refine   grid (6 nb nb, groups), nb = ceil(Ns / 8): one 256-thread workgroup per
//           8 x 8 block of coarse cells of a panel (ragged at the panel end) and per
//           group of rows: a kind-0 row with the rows that name it as their depth
//           (h, its momentum triple, its tracer masses: up to 8 slots).
//           stage    the 10 x 10 window of every slot into LDS as the reconstructed
//                    scalar (the row, M / h, hq / h): the block and one ring of real
//                    cells, those across a cube edge through the neighbour table.
//                    Window corners beyond a cube corner are never read.
//           phase 1  64 threads per slot, four slots at a time: thread p owns parent
//                    p.  It forms G from the four differences and the weight table,
//                    the min / max of the five cells, and walks its r r children in
//                    the fold's order for the mean correction and the extreme d_c;
//                    from those phi.  Coefficients (s_P, G, mean, phi, min, max) go
//                    to LDS.  A tracer slot's thread walks the children once more
//                    for delta, evaluating h_c and q_c from the coefficients with
//                    the expressions phase 2 uses, so the bits agree.
//           phase 2  the workgroup is re-dealt over the 8r x 8r children, child
//                    k 256 + tid of the block in row-major order (1, 4 or 16 per
//                    thread): consecutive lanes store consecutive fine cells of one
//                    row.  A child evaluates h_c, projects v_c at its own centre,
//                    forms M_c = h_c v_c and hq_c = h_c (q_c + delta), and stores
//                    through the padded map; a cell the rank does not own is skipped.
//  coarsen  grid 6 nb nb, nb = ceil(N / 16): one workgroup per 16 x 16 coarse block.
//           For every row and every child row cy the 16 fine rows of that cy are
//           loaded coalesced into an LDS stripe [16][16 r]; the coarse cell's thread
//           adds its r columns from there, so the fold's order holds and no thread
//           walks strided global memory.  A momentum triple is projected at the
//           parent's centre when its third row is done.
//
// All arithmetic is float64 with contraction off; stores are in the state's type.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LB = 256;
constexpr int PB = 8;        // parents per refine block edge
constexpr int WW = PB + 2;   // window edge
constexpr int MAXS = 8;      // slots of a group
constexpr int MAXF = 32;
constexpr int CB = 16;       // coarse cells per coarsen block edge
constexpr int NCF = 9;       // coefficients: s_P, G0, G1, G2, mean, phi, min, max, delta

struct Groups {
  int ng;
  unsigned char nslot[MAXF];
  unsigned char field[MAXF][MAXS];
  unsigned char kind[MAXF][MAXS];
};

// the child value of slot s, parent p at offset e = c_c - c_P
__device__ __forceinline__ double child(const double (*cf)[NCF][PB * PB], int s, int p, const double* e, int lim) {
  const double d = ((cf[s][1][p] * e[0] + cf[s][2][p] * e[1]) + cf[s][3][p] * e[2]) - cf[s][4][p];
  double v = cf[s][0][p] + cf[s][5][p] * d;
  if (lim) v = fmin(fmax(v, cf[s][6][p]), cf[s][7][p]);
  return v;
}

template <typename T, int R>
__global__ __launch_bounds__(LB) void transfer_refine_kernel(const TransferDesc d, const Groups G) {
  __shared__ double win[MAXS][WW * WW];
  __shared__ double cf[MAXS][NCF][PB * PB];
  const int Ns = d.Ns, N = d.N, tid = threadIdx.x;
  const int nb = (Ns + PB - 1) / PB;
  const int panel = blockIdx.x / (nb * nb), by = (blockIdx.x / nb) % nb, bx = blockIdx.x % nb;
  const int g = blockIdx.y, ns = G.nslot[g];
  const size_t Ks = (size_t)Ns * Ns, Ks6 = 6 * Ks, Kt = (size_t)N * N, Kt6 = 6 * Kt;
  const int f0 = G.field[g][0];

  // ---- stage: the reconstructed scalar of every slot on the 10 x 10 window
  for (int idx = tid; idx < ns * WW * WW; idx += LB) {
    const int s = idx / (WW * WW), w = idx % (WW * WW);
    const int gj = by * PB + w / WW - 1, gi = bx * PB + w % WW - 1;
    const int cj = min(max(gj, 0), Ns - 1), ci = min(max(gi, 0), Ns - 1);
    const int off = abs(gj - cj) + abs(gi - ci);
    double v = 0.0;
    if (off <= 1) {
      size_t cell = (size_t)panel * Ks + (size_t)cj * Ns + ci;
      if (off) cell = (size_t)d.nbr[4 * cell + (gi < 0 ? 0 : gi >= Ns ? 1 : gj < 0 ? 2 : 3)];
      v = d.src[(size_t)G.field[g][s] * Ks6 + cell];
      if (G.kind[g][s]) {
        const double h = d.src[(size_t)f0 * Ks6 + cell];
        v = h != 0.0 ? v / h : 0.0;
      }
    }
    win[s][w] = v;
  }
  __syncthreads();

  // ---- phase 1: coefficients of parent p of slot s
  const int p = tid % (PB * PB), pj = by * PB + p / PB, pi = bx * PB + p % PB;
  const bool pon = pj < Ns && pi < Ns;
  const size_t pcell = (size_t)panel * Ks + (size_t)pj * Ns + pi;
  double cP[3] = {0.0, 0.0, 0.0};
  if (pon) {
#pragma unroll
    for (int c = 0; c < 3; ++c) cP[c] = d.ctr_s[c * Ks6 + pcell];
  }
  for (int s0 = 0; s0 < ns; s0 += LB / (PB * PB)) {
    const int s = s0 + tid / (PB * PB);
    if (s >= ns || !pon) continue;
    const int w = (p / PB + 1) * WW + p % PB + 1;
    const double qP = win[s][w], qW = win[s][w - 1], qE = win[s][w + 1], qS = win[s][w - WW], qN = win[s][w + WW];
    const double dW = qW - qP, dE = qE - qP, dS = qS - qP, dN = qN - qP;
    double Gv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Gv[c] = ((d.W[c * Ks6 + pcell] * dW + d.W[(3 + c) * Ks6 + pcell] * dE) + d.W[(6 + c) * Ks6 + pcell] * dS) +
              d.W[(9 + c) * Ks6 + pcell] * dN;
    const double lo = fmin(qP, fmin(fmin(qW, qE), fmin(qS, qN))), hi = fmax(qP, fmax(fmax(qW, qE), fmax(qS, qN)));
    double sa = 0.0, sad = 0.0, dmax = -INFINITY, dmin = INFINITY;
    for (int cy = 0; cy < R; ++cy)
      for (int cx = 0; cx < R; ++cx) {
        const size_t tc = (size_t)(pj * R + cy) * N + (pi * R + cx);
        const double a = d.area_t[tc];
        double e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = d.ctr_t[c * Kt6 + panel * Kt + tc] - cP[c];
        const double dc = (Gv[0] * e[0] + Gv[1] * e[1]) + Gv[2] * e[2];
        sa = sa + a;
        sad = sad + a * dc;
        dmax = fmax(dmax, dc);
        dmin = fmin(dmin, dc);
      }
    const double m = sad / sa;
    dmax = dmax - m;
    dmin = dmin - m;
    double phi = 1.0;
    if (d.limiter) {
      const double pmax = dmax > 0.0 ? (hi - qP) / dmax : 1.0, pmin = dmin < 0.0 ? (lo - qP) / dmin : 1.0;
      phi = fmin(1.0, fmin(pmax, pmin));
      if (dmax == 0.0 && dmin == 0.0) phi = 0.0;
    }
    cf[s][0][p] = qP;
    cf[s][1][p] = Gv[0];
    cf[s][2][p] = Gv[1];
    cf[s][3][p] = Gv[2];
    cf[s][4][p] = m;
    cf[s][5][p] = phi;
    cf[s][6][p] = lo;
    cf[s][7][p] = hi;
    cf[s][8][p] = 0.0;
  }
  __syncthreads();
  // ---- phase 1, tracer slots: delta from the fold of a_c h_c q_c over the parent's children
  for (int s0 = 0; s0 < ns; s0 += LB / (PB * PB)) {
    const int s = s0 + tid / (PB * PB);
    if (s >= ns || !pon || G.kind[g][s] != 2) continue;
    double sa = 0.0, sw = 0.0, st = 0.0;
    for (int cy = 0; cy < R; ++cy)
      for (int cx = 0; cx < R; ++cx) {
        const size_t tc = (size_t)(pj * R + cy) * N + (pi * R + cx);
        const double a = d.area_t[tc];
        double e[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = d.ctr_t[c * Kt6 + panel * Kt + tc] - cP[c];
        const double wgt = a * child(cf, 0, p, e, d.limiter);
        sa = sa + a;
        sw = sw + wgt;
        st = st + wgt * child(cf, s, p, e, d.limiter);
      }
    cf[s][8][p] = sw != 0.0 ? (sa * d.src[(size_t)G.field[g][s] * Ks6 + pcell] - st) / sw : 0.0;
  }
  __syncthreads();

  // ---- phase 2: the children, row-major over the block's 8r x 8r fine cells
  constexpr int CPT = R * R / 4, FW = PB * R;
  T* Q = (T*)d.Q;
#pragma unroll 1
  for (int k = 0; k < CPT; ++k) {
    const int idx = k * LB + tid, fy = idx / FW, fx = idx % FW;
    const int q = (fy / R) * PB + fx / R;
    if (by * PB + fy / R >= Ns || bx * PB + fx / R >= Ns) continue;
    const size_t tc = (size_t)panel * Kt + (size_t)(by * FW + fy) * N + (bx * FW + fx);
    const int dst = d.padmap[tc];
    if (dst < 0) continue;
    const size_t qcell = (size_t)panel * Ks + (size_t)(by * PB + fy / R) * Ns + (bx * PB + fx / R);
    double c[3], e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[a] = d.ctr_t[a * Kt6 + tc];
      e[a] = c[a] - d.ctr_s[a * Ks6 + qcell];
    }
    const double hc = child(cf, 0, q, e, d.limiter);
    Q[(size_t)f0 * d.S + dst] = (T)hc;
    for (int s = 1; s < ns;) {
      if (G.kind[g][s] == 1) {
        const double vx = child(cf, s, q, e, d.limiter), vy = child(cf, s + 1, q, e, d.limiter),
                     vz = child(cf, s + 2, q, e, d.limiter);
        const double dn = (vx * c[0] + vy * c[1]) + vz * c[2];
        Q[(size_t)G.field[g][s] * d.S + dst] = (T)(hc * (vx - dn * c[0]));
        Q[(size_t)G.field[g][s + 1] * d.S + dst] = (T)(hc * (vy - dn * c[1]));
        Q[(size_t)G.field[g][s + 2] * d.S + dst] = (T)(hc * (vz - dn * c[2]));
        s += 3;
      } else {
        Q[(size_t)G.field[g][s] * d.S + dst] = (T)(hc * (child(cf, s, q, e, d.limiter) + cf[s][8][q]));
        s += 1;
      }
    }
  }
}

template <typename T, int R>
__global__ __launch_bounds__(LB) void transfer_coarsen_kernel(const TransferDesc d) {
  __shared__ double st[CB][CB * R + 1];
  const int Ns = d.Ns, N = d.N, tid = threadIdx.x;
  const int nb = (N + CB - 1) / CB;
  const int panel = blockIdx.x / (nb * nb), by = (blockIdx.x / nb) % nb, bx = blockIdx.x % nb;
  const int ty = tid / CB, tx = tid % CB, gj = by * CB + ty, gi = bx * CB + tx;
  const bool on = gj < N && gi < N;
  const size_t Ks = (size_t)Ns * Ns, Ks6 = 6 * Ks, Kt = (size_t)N * N, Kt6 = 6 * Kt;
  const size_t tc = (size_t)panel * Kt + (size_t)gj * N + gi;
  const int dst = on ? d.padmap[tc] : -1;
  double sa = 0.0;
  if (on)
    for (int cy = 0; cy < R; ++cy)
      for (int cx = 0; cx < R; ++cx) sa = sa + d.area_s[(size_t)(gj * R + cy) * Ns + (gi * R + cx)];
  T* Q = (T*)d.Q;
  double m0 = 0.0, m1 = 0.0;
  int t3 = 0;
  for (int f = 0; f < d.F; ++f) {
    double acc = 0.0;
    for (int cy = 0; cy < R; ++cy) {
      __syncthreads();
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int idx = k * LB + tid, row = idx / (CB * R), col = idx % (CB * R);
        const int fj = (by * CB + row) * R + cy, fi = bx * CB * R + col;
        st[row][col] = (fj < Ns && fi < Ns) ? d.src[(size_t)f * Ks6 + panel * Ks + (size_t)fj * Ns + fi] : 0.0;
      }
      __syncthreads();
      if (on)
#pragma unroll
        for (int cx = 0; cx < R; ++cx)
          acc = acc + d.area_s[(size_t)(gj * R + cy) * Ns + (gi * R + cx)] * st[ty][tx * R + cx];
    }
    const double mean = on ? acc / sa : 0.0;
    if (d.kind[f] != 1) {
      if (dst >= 0) Q[(size_t)f * d.S + dst] = (T)mean;
    } else if (t3 == 0) {
      m0 = mean;
      t3 = 1;
    } else if (t3 == 1) {
      m1 = mean;
      t3 = 2;
    } else {
      t3 = 0;
      if (dst >= 0) {
        const double c0 = d.ctr_t[tc], c1 = d.ctr_t[Kt6 + tc], c2 = d.ctr_t[2 * Kt6 + tc];
        const double dn = (m0 * c0 + m1 * c1) + mean * c2;
        Q[(size_t)(f - 2) * d.S + dst] = (T)(m0 - dn * c0);
        Q[(size_t)(f - 1) * d.S + dst] = (T)(m1 - dn * c1);
        Q[(size_t)f * d.S + dst] = (T)(mean - dn * c2);
      }
    }
  }
}

template <typename T, int R>
void launch_r(const TransferDesc* d, const Groups& G, hipStream_t s) {
  if (d->coarsen) {
    const int nb = (d->N + CB - 1) / CB;
    hipLaunchKernelGGL((transfer_coarsen_kernel<T, R>), dim3(6 * nb * nb), dim3(LB), 0, s, *d);
  } else {
    const int nb = (d->Ns + PB - 1) / PB;
    hipLaunchKernelGGL((transfer_refine_kernel<T, R>), dim3(6 * nb * nb, G.ng), dim3(LB), 0, s, *d, G);
  }
}

template <typename T>
int launch(const TransferDesc* d, const Groups& G, hipStream_t s) {
  if (d->r == 2) launch_r<T, 2>(d, G, s);
  if (d->r == 4) launch_r<T, 4>(d, G, s);
  if (d->r == 8) launch_r<T, 8>(d, G, s);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_transfer_desc_size(void) { return (int)sizeof(TransferDesc); }

// 0 ok; 1 bad pointers / shapes; 2 bad dtype; 3 launch error; 4 bad ratio; 5 inconsistent
// channel kinds; 6 depth index out of range
extern "C" int stsp_transfer_launch(int dtype, const TransferDesc* d, hipStream_t stream) {
  if (!d || !d->src || !d->Q || !d->padmap || !d->ctr_t || !d->area_s) return 1;
  if (d->Ns < 1 || d->N < 1 || d->F < 1 || d->F > MAXF || (d->coarsen & ~1) || (d->limiter & ~1)) return 1;
  if (d->r != 2 && d->r != 4 && d->r != 8) return 4;
  if (d->coarsen ? d->Ns != d->r * d->N : d->N != d->r * d->Ns) return 4;
  if (6ll * d->Ns * d->Ns >= (1ll << 31) || 6ll * d->N * d->N >= (1ll << 31) || d->S < 1) return 1;
  if (!d->coarsen && (!d->nbr || !d->W || !d->ctr_s || !d->area_t)) return 1;
  Groups G = {};
  int slot_of[MAXF];
  for (int f = 0; f < d->F; ++f) {
    if (d->kind[f] < 0 || d->kind[f] > 2) return 5;
    if (d->kind[f] == 0) {
      slot_of[f] = G.ng;
      G.field[G.ng][0] = (unsigned char)f;
      G.nslot[G.ng++] = 1;
    }
  }
  for (int f = 0; f < d->F;) {
    const int k = d->kind[f];
    if (k == 0) {
      ++f;
      continue;
    }
    const int len = k == 1 ? 3 : 1, h = d->depth[f];
    if (h < 0 || h >= d->F) return 6;
    if (d->kind[h] != 0 || f + len > d->F) return 5;
    const int g = slot_of[h];
    if (G.nslot[g] + len > MAXS) return 5;
    for (int a = 0; a < len; ++a) {
      if (d->kind[f + a] != k) return 5;
      if (d->depth[f + a] != h) return d->depth[f + a] < 0 || d->depth[f + a] >= d->F ? 6 : 5;
      G.field[g][G.nslot[g]] = (unsigned char)(f + a);
      G.kind[g][G.nslot[g]++] = (unsigned char)k;
    }
    f += len;
  }
  if (dtype == 1) return launch<double>(d, G, stream);
  if (dtype == 0) return launch<float>(d, G, stream);
  return 2;
}
