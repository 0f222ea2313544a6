// Shallow water with passive tracers: one RK stage per launch, gfx950 (CDNA4).
//
// State (h, M, hq_0 .. hq_{NQ-1}), 1 <= NQ <= 4 (models/swe.py::
// ShallowWaterTracers is the twin).  The SWE part is the arithmetic of
// stage_kernel.hip (physics 2, PLR faces fused into the flux phase); tracer k is
// reconstructed as the primitive q_k = hq_k / h with the same limiter and the
// same panel-edge treatment, and its edge flux is the SWE depth flux times the
// upwind face value,  F_hq = F_h (F_h > 0 ? qL : qR),  so that sum(hq A) is
// conserved to rounding and q = const stays constant.  No source term and no
// tangent projection for the tracers.
//
// A plainer kernel than stage_kernel.hip, whose role map is built for 1 or 4
// fields: thread e is edge e (x-edges, then y-edges), thread o < BX BY loads and
// updates own cell o, the next threads load one cell each of the two-cell ring
// around the block; the panel-edge
// fix-up runs block-wide, one (field, side, strip cell) per thread and pass.
// Push map, carried corner ghosts (cpush / cgmap), partial blocks and the
// block_sides rule are those of stage_kernel.hip.  No xGMI, no stamps.
//
// TLIM, the tracers' reconstruction, is "same as LIM" (0) or the monotone PPM
// (4, ShallowWaterTracers(tracer_limiter="ppm")): the mixing ratios alone go
// through PPM whose interface values are confined between their two cells
// before the Colella-Woodward limiter, (h, v) keep LIM.  The window then has
// three ghost layers (NG is a template value), the tracer faces are formed in
// the flux phase from six window cells per edge (no face arrays in LDS), and
// the panel-edge fix-up interpolates ghost layers 0 and 1 of the tracer rows
// (layer 0 only of the SWE rows) and builds the neighbour's tracer edge state
// on the six-cell line of models/base.py::_inner_face.
//
// NQ is a launch argument, not a template parameter (96 instantiations: fp64 /
// fp32, 16x16 / 16x8, limiters 0-3, tracers as LIM / PPM, plain / block list /
// block list + remote ghosts).  LDS is dynamic, sized by NQ (TrGeom::elems), AND
// the flux array is reused: it holds F_h, F_M and the flux of tracer 0 (5 rows);
// tracers 1 .. 3 wait in registers and go through rows 1 .. 3 in a second pass
// once the momentum fluxes are consumed.  16x16 fp64 with NQ = 4: 63 824 bytes,
// under the 64 KiB a launch gets without opting in; with PPM tracers 70 016
// bytes, which the launcher refuses (NQ <= 3: 65 456; 16x8 with NQ = 4: 43 904).
#include "stage_common.h"

namespace {

constexpr int TR_MAXQ = 4;
constexpr int TR_PPM = 4;     // TLIM: monotone PPM for the mixing ratios (0: same as LIM)
constexpr int tr_ng(int tlim) { return tlim == TR_PPM ? 3 : 2; }   // ghost layers

// NG ghost layers; the fix-up interpolates layer 0 of every field and, with
// NG = 3, layer 1 of the tracer rows
template <int BX, int BY, int NG> struct TrGeom {
  static constexpr int NX = (BX + 1) * BY, NY = BX * (BY + 1), NE = NX + NY;
  static constexpr int NT = ((NE + 63) / 64) * 64;
  static constexpr int EX = BX + 2 * NG, EY = BY + 2 * NG;
  static constexpr int WS = EX + 1, WF = EY * WS;      // window row / field stride
  static constexpr int BM = BX > BY ? BX : BY, EM = EX > EY ? EX : EY;
  static constexpr int NB = BX + BY + 2;               // normals: x columns, then y rows
  static constexpr int FLR = 5;                        // flux rows
  // window (h, v, c, q_k) | fluxes | neighbour edge state | neighbour raw cell | normals | lengths
  static constexpr int elems(int nq) {
    return (5 + nq) * WF + FLR * NE + (4 + nq) * 4 * BM + 5 * 4 * BM + 3 * NB + NE;
  }
  static_assert(EX * EY <= NT, "one window cell per thread");
  static_assert(3 * NB <= NT, "one normal component per thread");
  // raw strip copy: layer 0 of all 4 + NQ fields, layer 1 of the NQ tracer rows (NG = 3)
  static constexpr int raw_rows(int nq) { return 4 + nq + (NG == 3 ? nq : 0); }
  static_assert(4 * raw_rows(TR_MAXQ) * EM <= FLR * NE, "the raw strip copy fits in the flux array");
};

// monotone PPM (models/base.py::ppm_faces, monotone): the fourth-order interface
// value between cells b and c of the line a b | c d, confined to [min, max](b, c)
template <typename T>
__device__ __forceinline__ T ppm_iface(T a, T b, T c, T d) {
  const T v = T(7.0 / 12.0) * (b + c) - T(1.0 / 12.0) * (a + d);
  return tmin(tmax(v, tmin(b, c)), tmax(b, c));
}
// Colella-Woodward monotonicity limiter of one cell (models/base.py::ppm_limit)
template <typename T>
__device__ __forceinline__ void ppm_limit(T c0, T aL, T aR, T& nL, T& nR) {
  const bool flat = (aR - c0) * (c0 - aL) <= T(0);
  const T d = aR - aL;
  const T m6 = T(6) * (c0 - T(0.5) * (aL + aR));
  const bool ovl = d * m6 > d * d;
  const bool ovr = -(d * d) > d * m6;
  nL = flat ? c0 : (ovl ? T(3) * c0 - T(2) * aR : aL);
  nR = flat ? c0 : ((!ovl && ovr) ? T(3) * c0 - T(2) * aL : aR);
}

template <typename T, int BX, int BY, int LIM, int TLIM, bool REMOTE, bool LIST>
__global__ __launch_bounds__((TrGeom<BX, BY, tr_ng(TLIM)>::NT)) void swe_tracer_kernel(Args<T> a, const int NQ) {
  constexpr int NG = tr_ng(TLIM);
  constexpr bool TPPM = TLIM == TR_PPM;
  constexpr int KG = TPPM ? 2 : 1;                // interpolated ghost layers (tracer rows)
  using G = TrGeom<BX, BY, NG>;
  constexpr int NT = G::NT, NX = G::NX, NY = G::NY, NE = G::NE;
  constexpr int EX = G::EX, EY = G::EY, WS = G::WS, WF = G::WF, BM = G::BM, EM = G::EM;
  extern __shared__ __align__(16) unsigned char tr_smem[];
  const int FR = 4 + NQ;                          // reconstructed fields = state fields
  T* const s_w = reinterpret_cast<T*>(tr_smem);   // [5 + NQ][EY][WS]: h, v (3), sqrt(g h), q_k
  T* const s_fl = s_w + (5 + NQ) * WF;            // [5][NE]
  T* const s_pf = s_fl + G::FLR * NE;             // [FR][4 BM] neighbour's edge state
  T* const s_pr = s_pf + FR * 4 * BM;             // [5][4 BM] neighbour's raw cell (h, v, c)
  T* const s_nrm = s_pr + 5 * 4 * BM;             // [3][NB]
  T* const s_len = s_nrm + 3 * G::NB;             // [NE]
  // raw ghosts (until the flux phase): [4][RR][EM], rows f < FR layer 0 of field
  // f, rows FR + k layer 1 of tracer k (PPM)
  T* const s_raw = s_fl;
  const int RR = FR + (KG - 1) * NQ;
  auto wfield = [](int f) { return f < 4 ? f : f + 1; };   // window row of reconstructed field f

  const int bid = LIST ? a.blocks[blockIdx.x] : xcd_remap(blockIdx.x, a.nblocks);
  const int n = a.n, S = a.S, nn = n * n, mg = a.mg, pw = a.pw;
  const int nbx = (n + BX - 1) / BX, nby = (n + BY - 1) / BY;
  const int tile = bid / (nbx * nby);
  const int rem = bid - tile * nbx * nby;
  const int yb = rem / nbx, xb = rem - yb * nbx;
  const int x0 = xb * BX, y0 = yb * BY;
  const int tid = threadIdx.x;
  const long tb = (long)tile * pw * pw;
  const int gbase = tile * nn;
  const int pe_word = a.pedge[tile];
  // sides of this block on a cube edge: a side counts as soon as the window
  // reaches its ghost strip (the last block may be one cell wide)
  const int bsides = (x0 == 0 ? (pe_word & 1) : 0) | (x0 + BX + NG > n ? (pe_word & 2) : 0) |
                     (y0 == 0 ? (pe_word & 4) : 0) | (y0 + BY + NG > n ? (pe_word & 8) : 0);

  // ---- 0. own cell operands ---------------------------------------------------
  const int ox = tid % BX, oy = tid / BX;
  const int cx = x0 + ox, cy = y0 + oy;
  const bool own = tid < BX * BY && cx < n && cy < n;
  const long pc = tb + (long)(cy + mg) * pw + (cx + mg);
  const bool need_x = (a.a0 != T(0)) || (a.acc_out && a.c1 != T(0));
  const bool need_acc = a.acc_out && a.acc_in && (a.c0 != T(0));
  T xs[4], qo[4], acs[4], txs[TR_MAXQ], tqo[TR_MAXQ], tacs[TR_MAXQ];
#pragma unroll
  for (int f = 0; f < 4; ++f) { xs[f] = qo[f] = acs[f] = T(0); txs[f] = tqo[f] = tacs[f] = T(0); }
  T iA = T(0), r0 = T(0), r1 = T(0), r2 = T(0);
  T gb[3] = {T(0), T(0), T(0)};
  int pt[4] = {-1, -1, -1, -1};
  if (own) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (need_x) xs[f] = a.X[(long)f * S + pc];
      if (need_acc) acs[f] = a.acc_in[(long)f * S + pc];
    }
    T rec[8];
    load_rec8<T>(a.cgeo + (long)(gbase + cy * n + cx) * 8, rec);
    iA = rec[0]; r0 = rec[1]; r1 = rec[2]; r2 = rec[3];
    gb[0] = rec[4]; gb[1] = rec[5]; gb[2] = rec[6];
    const int* pm = a.push + (long)tile * 4 * mg * n;
    if (cx < mg) pt[0] = pm[(0 * mg + cx) * n + cy];
    if (cx >= n - mg) pt[1] = pm[(1 * mg + (n - 1 - cx)) * n + cy];
    if (cy < mg) pt[2] = pm[(2 * mg + cy) * n + cx];
    if (cy >= n - mg) pt[3] = pm[(3 * mg + (n - 1 - cy)) * n + cx];
    // a cell of a tile-corner block may also feed a carried corner ghost
    // (layout: only when n >= 2 mg, so its x push on the far side is unused)
    if (a.cpush && (cx < mg || cx >= n - mg) && (cy < mg || cy >= n - mg)) {
      const int qx = cx < mg ? 0 : 1, qy = cy < mg ? 0 : 1;
      const int cb = qx ? n - 1 - cx : cx, ca = qy ? n - 1 - cy : cy;
      const int v = a.cpush[((tile * 4 + (qx | (qy << 1))) * mg + ca) * mg + cb];
      if (v != -1) pt[qx ^ 1] = v;
    }
  }
  // edge normals of this block's columns / rows: into a register now, into LDS
  // once the window loads are issued (an LDS store of a global load waits for
  // it, and every load issued before it: a round trip in front of the window)
  T nrm = T(0);
  int nrm_i = -1;
  if (tid < 3 * (BX + 1)) {
    const int k = tid / (BX + 1), c = tid - k * (BX + 1);
    nrm_i = k * G::NB + c;
    if (x0 + c <= n) nrm = a.mx[(tile * 3 + k) * (n + 1) + x0 + c];
  } else if (tid < 3 * G::NB) {
    const int u = tid - 3 * (BX + 1);
    const int k = u / (BY + 1), c = u - k * (BY + 1);
    nrm_i = k * G::NB + BX + 1 + c;
    if (y0 + c <= n) nrm = a.my[(tile * 3 + k) * (n + 1) + y0 + c];
  }
  // this thread's edge
  const int eid = tid;
  const bool is_x = eid < NX;
  const int ete = is_x ? eid : eid - NX;
  const int e_r = is_x ? ete / (BX + 1) : ete / BX;
  const int e_c = is_x ? ete - e_r * (BX + 1) : ete - e_r * BX;
  const int ex_ = x0 + e_c, ey_ = y0 + e_r;
  const bool edge_ok = is_x ? (ex_ <= n && ey_ < n) : (eid < NE && ex_ < n && ey_ <= n);
  T coef = T(0);
  if (edge_ok)
    coef = is_x ? a.ex[(long)tile * n * (n + 1) + ey_ * (n + 1) + ex_] : a.ey[(long)tile * (n + 1) * n + ey_ * n + ex_];

  // ---- 1. window (block + 2 ghost layers) -> LDS as primitives ------------------
  // Thread o < BX BY loads its own cell (and keeps the conserved values for the
  // update), the next RING threads one cell each of the two-cell ring around
  // the block: NG rows below and above, then NG columns left and right.
  constexpr int NIN = BX * BY, RING = EX * EY - NIN;
  int ly = -1, lx = 0;
  if (tid < NIN) {
    ly = NG + oy; lx = NG + ox;
  } else if (tid - NIN < 2 * NG * EX) {
    const int r = tid - NIN, rr = r / EX;
    lx = r - rr * EX;
    ly = rr < NG ? rr : EY - 2 * NG + rr;
  } else if (tid - NIN < RING) {
    const int r2 = tid - NIN - 2 * NG * EX, rr = r2 / (2 * NG), c = r2 - rr * (2 * NG);
    ly = NG + rr;
    lx = c < NG ? c : EX - 2 * NG + c;
  }
  if (ly >= 0) {
    const int x = x0 + lx - NG, y = y0 + ly - NG;
    T v[4] = {T(0), T(0), T(0), T(0)}, tq[TR_MAXQ] = {T(0), T(0), T(0), T(0)};
    if (x < n + NG && y < n + NG) {          // false only past a partial block
      int m = 0;                             // < 0: remote slot -1 - m
      if constexpr (REMOTE) {
        const bool oxx = (x < 0) | (x >= n), oyy = (y < 0) | (y >= n);
        if (oxx != oyy) {
          int side, layer, pos;
          if (x < 0) { side = 0; layer = -1 - x; pos = y; }
          else if (x >= n) { side = 1; layer = x - n; pos = y; }
          else if (y < 0) { side = 2; layer = -1 - y; pos = x; }
          else { side = 3; layer = y - n; pos = x; }
          m = a.gmap[((tile * 4 + side) * mg + layer) * n + pos];
        } else if (oxx && a.cgmap) {         // a tile-corner ghost: carried ones may be remote
          const int ca = y < 0 ? -1 - y : y - n, cb = x < 0 ? -1 - x : x - n;
          m = a.cgmap[((tile * 4 + (x >= n ? 1 : 0) + (y >= n ? 2 : 0)) * mg + ca) * mg + cb];
        }
      }
      if (m < 0) {
        const T* rp = a.recv + (long)(-1 - m) * FR;
#pragma unroll
        for (int f = 0; f < 4; ++f) v[f] = rp[f];
#pragma unroll
        for (int k = 0; k < TR_MAXQ; ++k)
          if (k < NQ) tq[k] = rp[4 + k];
      } else {
        const long pa = tb + (long)(y + mg) * pw + (x + mg);
#pragma unroll
        for (int f = 0; f < 4; ++f) v[f] = a.Q[(long)f * S + pa];
#pragma unroll
        for (int k = 0; k < TR_MAXQ; ++k)
          if (k < NQ) tq[k] = a.Q[(long)(4 + k) * S + pa];
      }
    }
    if (nrm_i >= 0) s_nrm[nrm_i] = nrm;
    if (edge_ok) s_len[eid] = coef;
    if (own) {
#pragma unroll
      for (int f = 0; f < 4; ++f) { qo[f] = v[f]; tqo[f] = tq[f]; }
    }
    const T inv = v[0] != T(0) ? trcp(v[0]) : T(0);
    const int wi = ly * WS + lx;
    T w[4 + TR_MAXQ];
    w[0] = v[0]; w[1] = v[1] * inv; w[2] = v[2] * inv; w[3] = v[3] * inv;
#pragma unroll
    for (int k = 0; k < TR_MAXQ; ++k) w[4 + k] = tq[k] * inv;
#pragma unroll
    for (int f = 0; f < 4; ++f) s_w[f * WF + wi] = w[f];
    s_w[4 * WF + wi] = tsqrt(a.g * tmax(v[0], T(0)));
#pragma unroll
    for (int k = 0; k < TR_MAXQ; ++k)
      if (k < NQ) s_w[(5 + k) * WF + wi] = w[4 + k];
    if (bsides) {   // a raw panel-edge ghost (layer 0) the fix-up interpolates from
      const bool inx = (x >= 0) & (x < n), iny = (y >= 0) & (y < n);
      // strip cells, and the tile-corner cells beyond the strip ends (carried
      // corner ghosts): filed under the side that is a panel edge
      int side = -1, k = 0, al = 0;
      if (!inx) {
        side = x < 0 ? 0 : 1; k = x < 0 ? -1 - x : x - n; al = ly;
        if (!(k < KG && ((bsides >> side) & 1))) side = -1;
      }
      if (side < 0 && !iny) { side = y < 0 ? 2 : 3; k = y < 0 ? -1 - y : y - n; al = lx; }
      if (side >= 0 && k < KG && ((bsides >> side) & 1) && !(inx && iny)) {
        if (!TPPM || k == 0) {
#pragma unroll
          for (int f = 0; f < 4 + TR_MAXQ; ++f)
            if (f < FR) s_raw[(side * RR + f) * EM + al] = w[f];
        } else {
#pragma unroll
          for (int q = 0; q < TR_MAXQ; ++q)
            if (q < NQ) s_raw[(side * RR + FR + q) * EM + al] = w[4 + q];
        }
      }
    }
  } else {
    if (nrm_i >= 0) s_nrm[nrm_i] = nrm;
    if (edge_ok) s_len[eid] = coef;
  }
  __syncthreads();

  // ---- 1a. panel edges: interpolated ghosts + the neighbour's edge state --------
  // (models/base.py::reconstruct; the block-wide form of stage_kernel.hip 1a)
  if (bsides) {   // block-uniform
    for (int u = tid; u < FR * 4 * BM; u += NT) {
      const int f = u / (4 * BM), r4 = u - f * (4 * BM);
      const int pside = r4 / BM, pjl = r4 - pside * BM;
      const int pj = (pside < 2 ? y0 : x0) + pjl;            // strip cell, tile-local
      if (!(pjl < (pside < 2 ? BY : BX) && pj < n && ((bsides >> pside) & 1))) continue;
      const int ti = ((tile * 4 + pside) * 3 + 0) * n + pj;
      const int pb = a.pe_base[ti];
      const T ptt = a.pe_t[ti];
      const bool plow = (pside & 1) == 0;
      auto widx = [&](int cn, int al) {  // window index of (normal coord, along coord), tile-local
        const int x = pside < 2 ? cn : al, y = pside < 2 ? al : cn;
        return (y - y0 + NG) * WS + (x - x0 + NG);
      };
      const int pab = (pside < 2 ? y0 : x0) - NG;            // tile-local coordinate of window position 0
      T* const wf = s_w + wfield(f) * WF;
      const T* const raw = s_raw + (pside * RR + f) * EM;
      const T g0 = raw[pb - pab], g1 = raw[pb + 1 - pab];
      const T gk = g0 + ptt * (g1 - g0);
      const int co = plow ? 0 : n - 1;
      const T o0 = wf[widx(co, pb)], o1 = wf[widx(co, pb + 1)];
      const T l = o0 + ptt * (o1 - o0);
      const T c = raw[pj - pab];
      const int wend = (pside < 2 ? x0 + BX : y0 + BY) + NG;   // first coordinate past the window
      // PPM: the block that holds the panel edge itself uses the neighbour's
      // state; a block whose window merely reaches the strip (NG cells short of
      // the edge) only needs the ghosts, and its window ends before raw layer 2
      const bool pown = !TPPM || plow || n + NG <= wend;
      T nf = T(0);
      if (TPPM && f >= 4) {
        // layer 1 with its own pair; the neighbour's face on the line
        // [gp1, gp0 | raw0, raw1, raw2] (gp2 is not read)
        const int pb1 = a.pe_base[ti + n];
        const T pt1 = a.pe_t[ti + n];
        const T* const raw1 = s_raw + (pside * RR + FR + (f - 4)) * EM;
        const T h0 = raw1[pb1 - pab], h1 = raw1[pb1 + 1 - pab];
        const T gk1 = h0 + pt1 * (h1 - h0);
        if (pown) {
          const int co1 = plow ? 1 : n - 2;
          const T u0 = wf[widx(co1, pb1)], u1 = wf[widx(co1, pb1 + 1)];
          const T l2 = u0 + pt1 * (u1 - u0);
          const T r = raw1[pj - pab];
          const T r2 = wf[widx(plow ? -3 : n + 2, pj)];
          T nR;
          ppm_limit<T>(c, ppm_iface<T>(l2, l, c, r), ppm_iface<T>(l, c, r, r2), nf, nR);
        }
        if (plow || n + 1 < wend) wf[widx(plow ? -2 : n + 1, pj)] = gk1;
      } else if (pown) {
        const T r = wf[widx(plow ? -2 : n + 1, pj)];
        nf = c - half_slope<LIM>(c - l, r - c);
      }
      if (plow || n < wend) wf[widx(plow ? -1 : n, pj)] = gk;
      if (!pown) continue;
      const int pslt = pside * BM + pjl;
      s_pf[f * 4 * BM + pslt] = nf;
      if (f < 4) s_pr[f * 4 * BM + pslt] = c;
      if (f == 0) s_pr[4 * 4 * BM + pslt] = s_w[4 * WF + widx(plow ? -1 : n, pj)];   // raw sound speed
    }
    __syncthreads();
  }

  // ---- 2. one edge flux per thread ----------------------------------------------
  int pslot = -1;
  bool plo = false;
  if (bsides && edge_ok) {
    if (is_x && ex_ == 0 && (bsides & 1)) { pslot = 0 * BM + ey_ - y0; plo = true; }
    else if (is_x && ex_ == n && (bsides & 2)) { pslot = 1 * BM + ey_ - y0; }
    else if (!is_x && ey_ == 0 && (bsides & 4)) { pslot = 2 * BM + ex_ - x0; plo = true; }
    else if (!is_x && ey_ == n && (bsides & 8)) { pslot = 3 * BM + ex_ - x0; }
  }
  T tfl[TR_MAXQ] = {T(0), T(0), T(0), T(0)};   // tracer fluxes of this edge
  if (edge_ok) {
    const int cl_ = is_x ? (NG + e_r) * WS + NG - 1 + e_c : (NG - 1 + e_r) * WS + NG + e_c;
    const int cst = is_x ? 1 : WS;
    T wl[4], wr[4], cl[5], cr[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) { cl[f] = s_w[f * WF + cl_]; cr[f] = s_w[f * WF + cl_ + cst]; }
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const T m1 = s_w[f * WF + cl_ - cst], p2 = s_w[f * WF + cl_ + 2 * cst];
      const T d1 = cr[f] - cl[f];
      wl[f] = cl[f] + half_slope<LIM>(cl[f] - m1, d1);
      wr[f] = cr[f] - half_slope<LIM>(d1, p2 - cr[f]);
    }
    if (pslot >= 0) {   // panel edge: the neighbour's state and raw cell
      if (plo) {
#pragma unroll
        for (int f = 0; f < 4; ++f) wl[f] = s_pf[f * 4 * BM + pslot];
#pragma unroll
        for (int f = 0; f < 5; ++f) cl[f] = s_pr[f * 4 * BM + pslot];
      } else {
#pragma unroll
        for (int f = 0; f < 4; ++f) wr[f] = s_pf[f * 4 * BM + pslot];
#pragma unroll
        for (int f = 0; f < 5; ++f) cr[f] = s_pr[f * 4 * BM + pslot];
      }
    }
    const int ni = is_x ? e_c : BX + 1 + e_r;
    T fl[4];
    swe_flux<T>(wl, wr, cl, cr, s_nrm[ni], s_nrm[G::NB + ni], s_nrm[2 * G::NB + ni], coef, a.g, fl);
    // tracers: upwind face value on the depth flux
#pragma unroll
    for (int k = 0; k < TR_MAXQ; ++k) {
      if (k < NQ) {
        const T* wq = s_w + (5 + k) * WF;
        const T m1 = wq[cl_ - cst], c0 = wq[cl_], p1 = wq[cl_ + cst], p2 = wq[cl_ + 2 * cst];
        T ql, qr;
        if constexpr (TPPM) {
          // the three interfaces around the left and the right cell, then aR of
          // the left and aL of the right cell
          const T m2 = wq[cl_ - 2 * cst], p3 = wq[cl_ + 3 * cst];
          const T ia = ppm_iface<T>(m2, m1, c0, p1), ib = ppm_iface<T>(m1, c0, p1, p2);
          const T ic = ppm_iface<T>(c0, p1, p2, p3);
          T dum;
          ppm_limit<T>(c0, ia, ib, dum, ql);
          ppm_limit<T>(p1, ib, ic, qr, dum);
        } else {
          const T d1 = p1 - c0;
          ql = c0 + half_slope<LIM>(c0 - m1, d1);
          qr = p1 - half_slope<LIM>(d1, p2 - p1);
        }
        if (pslot >= 0) {
          const T pv = s_pf[(4 + k) * 4 * BM + pslot];
          if (plo) ql = pv; else qr = pv;
        }
        tfl[k] = fl[0] * (fl[0] > T(0) ? ql : qr);
      }
    }
    // (the raw strip copy that shared the flux array is dead: the fix-up
    // finished before the barrier above)
#pragma unroll
    for (int f = 0; f < 4; ++f) s_fl[f * NE + eid] = fl[f];
    s_fl[4 * NE + eid] = tfl[0];
  }
  // the tracers' own-cell operands are issued here, not with the SWE ones in
  // phase 0: held across the flux phase they cost up to 24 VGPRs there (fp64),
  // which is what decides the waves per SIMD; their latency hides under the
  // sources and the barrier
  if (own) {
#pragma unroll
    for (int k = 0; k < TR_MAXQ; ++k) {
      if (k < NQ) {
        if (need_x) txs[k] = a.X[(long)(4 + k) * S + pc];
        if (need_acc) tacs[k] = a.acc_in[(long)(4 + k) * S + pc];
      }
    }
  }
  // own-cell terms that need no flux: sources and the RK base
  const int ew = oy * (BX + 1) + ox;            // west x-edge of the cell
  const int es = NX + oy * BX + ox;             // south y-edge
  T src[3] = {T(0), T(0), T(0)};
  if (own) {
    const T fc = a.omega2 * r2;
    const T h = qo[0];
    const T cor[3] = {r1 * qo[3] - r2 * qo[2], r2 * qo[1] - r0 * qo[3], r0 * qo[2] - r1 * qo[1]};
    // curvature balance g/2 h^2 sum(+-L m)/A: a constant depth is force-free
    const T Lw = s_len[ew], Le = s_len[ew + 1], Ls = s_len[es], Ln = s_len[es + BX];
    const T pb = T(0.5) * a.g * h * h * iA, gh = a.g * h;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const T* nk = s_nrm + k * G::NB;
      const T Sk = Le * nk[ox + 1] - Lw * nk[ox] + Ln * nk[BX + 2 + oy] - Ls * nk[BX + 1 + oy];
      src[k] = -fc * cor[k] + pb * Sk - gh * gb[k];
    }
  }
  __syncthreads();

  // ---- 3. divergence + RK combination + push ------------------------------------
  auto store = [&](T* base, int f, T v) {
    base[(long)f * S + pc] = v;
  };
  auto store_out = [&](int f, T v) {
    store(a.out, f, v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pt[k] >= 0) a.out[(long)f * S + pt[k]] = v;
  };
  // one tracer field from flux row `row`
  auto tracer_update = [&](int k, int row) {
    const T* fr = s_fl + row * NE;
    const T dq = -((fr[ew + 1] - fr[ew]) + (fr[es + BX] - fr[es])) * iA;
    T base = T(0);
    if (a.a1 != T(0)) base = a.a1 * tqo[k];
    if (a.a0 != T(0)) base += a.a0 * txs[k];
    const T o = a.a2 * a.dt * dq + base;
    if (a.acc_out) {
      T p = a.c2 * a.dt * dq;
      if (a.c1 != T(0)) p += a.c1 * txs[k];
      if (need_acc) p += a.c0 * tacs[k];
      store(a.acc_out, 4 + k, p);
    }
    store_out(4 + k, o);
  };
  if (own) {
    T dq[4], o[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const T* fr = s_fl + f * NE;
      dq[f] = -((fr[ew + 1] - fr[ew]) + (fr[es + BX] - fr[es])) * iA;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dq[1 + k] += src[k];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      T base = T(0);
      if (a.a1 != T(0)) base = a.a1 * qo[f];
      if (a.a0 != T(0)) base += a.a0 * xs[f];
      o[f] = a.a2 * a.dt * dq[f] + base;
    }
    {
      const T d = o[1] * r0 + o[2] * r1 + o[3] * r2;
      o[1] -= d * r0; o[2] -= d * r1; o[3] -= d * r2;
    }
    if (a.acc_out) {
      T p[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) p[f] = a.c2 * a.dt * dq[f];
      if (a.c1 != T(0)) {
#pragma unroll
        for (int f = 0; f < 4; ++f) p[f] += a.c1 * xs[f];
      }
      if (need_acc) {
#pragma unroll
        for (int f = 0; f < 4; ++f) p[f] += a.c0 * acs[f];
      }
      const T d = p[1] * r0 + p[2] * r1 + p[3] * r2;
      p[1] -= d * r0; p[2] -= d * r1; p[3] -= d * r2;
#pragma unroll
      for (int f = 0; f < 4; ++f) store(a.acc_out, f, p[f]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) store_out(f, o[f]);
    tracer_update(0, 4);
  }
  if (NQ > 1) {   // second pass: tracers 1 .. 3 through flux rows 1 .. 3
    __syncthreads();
    if (edge_ok) {
#pragma unroll
      for (int k = 1; k < TR_MAXQ; ++k)
        if (k < NQ) s_fl[k * NE + eid] = tfl[k];
    }
    __syncthreads();
    if (own) {
#pragma unroll
      for (int k = 1; k < TR_MAXQ; ++k)
        if (k < NQ) tracer_update(k, k);
    }
  }
}

template <typename T, int BX, int BY, int LIM, int TLIM>
int tr_launch_l(const StageDesc* d, hipStream_t s) {
  using G = TrGeom<BX, BY, tr_ng(TLIM)>;
  const Args<T> a = make_args<T>(d);
  const int nq = d->nq;
  const size_t lds = (size_t)G::elems(nq) * sizeof(T);
  if (lds > 65536) return -13;
  const dim3 grid(d->nblocks), block(G::NT);
  if (d->remote)
    hipLaunchKernelGGL((swe_tracer_kernel<T, BX, BY, LIM, TLIM, true, true>), grid, block, lds, s, a, nq);
  else if (d->blocks)
    hipLaunchKernelGGL((swe_tracer_kernel<T, BX, BY, LIM, TLIM, false, true>), grid, block, lds, s, a, nq);
  else
    hipLaunchKernelGGL((swe_tracer_kernel<T, BX, BY, LIM, TLIM, false, false>), grid, block, lds, s, a, nq);
  return (int)hipGetLastError();
}

template <typename T, int BX, int BY, int TLIM>
int tr_launch_t(const StageDesc* d, hipStream_t s) {
  if (d->nblocks <= 0) return 0;
  if (d->nq < 1 || d->nq > TR_MAXQ) return -14;
  if (d->pw != d->n + 2 * d->mg || d->mg < 2) return -5;
  if (d->mg < tr_ng(TLIM)) return -15;                                 // PPM tracers: three ghost layers
  if (!d->pedge || !d->pe_base || !d->pe_t || d->n < 2) return -12;   // panel-edge tables
  if (!d->mx || !d->my || !d->cgeo || !d->ex || !d->ey) return -6;
  if (!d->push || (d->remote && (!d->gmap || !d->blocks || !d->recv))) return -6;
  if (d->xg) return -10;                                               // no direct xGMI halo
  switch (d->limiter) {
    case 0: return tr_launch_l<T, BX, BY, 0, TLIM>(d, s);
    case 1: return tr_launch_l<T, BX, BY, 1, TLIM>(d, s);
    case 2: return tr_launch_l<T, BX, BY, 2, TLIM>(d, s);
    case 3: return tr_launch_l<T, BX, BY, 3, TLIM>(d, s);
    case 4: return -11;                                                // PPM for (h, v): not with tracers
  }
  return -7;
}

template <typename T>
int tr_launch_p(int bx, int by, const StageDesc* d, hipStream_t s) {
  if (d->tracer_limiter != 0 && d->tracer_limiter != TR_PPM) return -16;
  const bool ppm = d->tracer_limiter == TR_PPM;
  if (bx == 16 && by == 16) return ppm ? tr_launch_t<T, 16, 16, TR_PPM>(d, s) : tr_launch_t<T, 16, 16, 0>(d, s);
  if (bx == 16 && by == 8) return ppm ? tr_launch_t<T, 16, 8, TR_PPM>(d, s) : tr_launch_t<T, 16, 8, 0>(d, s);
  return -2;
}

}  // namespace

extern "C" int stsp_swe_tracer_launch(int dtype, int bx, int by, const StageDesc* d, hipStream_t stream) {
  if (dtype == 1) return tr_launch_p<double>(bx, by, d, stream);
  if (dtype == 0) return tr_launch_p<float>(bx, by, d, stream);
  return -4;
}

// dynamic LDS bytes of a launch (host-side contract check)
extern "C" int stsp_swe_tracer_lds(int dtype, int bx, int by, int nq) {
  const int es = dtype == 1 ? 8 : 4;
  if (bx == 16 && by == 16) return TrGeom<16, 16, 2>::elems(nq) * es;
  if (bx == 16 && by == 8) return TrGeom<16, 8, 2>::elems(nq) * es;
  return -1;
}

// the same for a tracer reconstruction (0: as the limiter, 4: monotone PPM on a
// three-layer window); a launch over 65536 bytes is refused with -13
extern "C" int stsp_swe_tracer_lds_tl(int dtype, int bx, int by, int nq, int tracer_limiter) {
  if (tracer_limiter == 0) return stsp_swe_tracer_lds(dtype, bx, by, nq);
  if (tracer_limiter != TR_PPM) return -1;
  const int es = dtype == 1 ? 8 : 4;
  if (bx == 16 && by == 16) return TrGeom<16, 16, 3>::elems(nq) * es;
  if (bx == 16 && by == 8) return TrGeom<16, 8, 3>::elems(nq) * es;
  return -1;
}
