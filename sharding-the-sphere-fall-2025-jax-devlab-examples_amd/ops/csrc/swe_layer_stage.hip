// Two-layer (stacked, isopycnal) shallow water: one RK stage per launch, gfx950
// (CDNA4).  models/swe.py::LayeredShallowWater with two layers is the twin.
//
// State (h_0, M_0, h_1, M_1), field-major; layer 0 is the top one and
// r = rho_0 / rho_1 <= 1.  Each layer is the shallow-water layer of
// stage_kernel.hip (physics 2: PLR faces fused into the flux phase, Rusanov
// flux, curvature balance, Coriolis, static -g h grad b, tangent projection)
// with two changes:
//   * the momentum source gains -g h_k grad(c_k), c_0 = h_1 (the layer below
//     lifts with weight 1), c_1 = r h_0 (the layer above presses with its
//     density ratio).  grad(c_k) is the Gauss sum over the four faces of
//     (cbar_face - c_cell) L m / A with the face's sign, projected onto the
//     tangent plane at the cell centre; cbar_face is the mean (hL + hR) / 2 of
//     the other layer's two edge states, the very states its flux uses, so the
//     value is the same from both sides of a cube edge.  c_cell is subtracted
//     before anything is multiplied: uniform layers give exactly zero and fp32
//     does not cancel large terms;
//   * the Rusanov speed of both layers is |v_k . m| + sqrt(g (h_0 + h_1)) of the
//     cell averages, which bounds the external and the internal wave speeds.
//
// Roles and tables are those of swe_tracer_stage.hip: thread e is edge e
// (x-edges, then y-edges), thread o < BX BY loads and updates own cell o, the
// next threads load one cell each of the two-cell ring around the block; the
// panel-edge fix-up runs block-wide, one (field, side, strip cell) per thread
// and pass.  Push map, carried corner ghosts (cpush / cgmap), partial blocks
// and the block_sides rule are those of stage_kernel.hip.  No xGMI, no stamps.
//
// LDS (dynamic): the window holds the eight primitives and one sqrt(g H) row
// shared by both layers.  The layers go through the five flux rows one after
// the other: each edge thread forms both layers' edge states once, one layer at
// a time (eight live edge-state values, not sixteen), writes layer 0's four
// fluxes and cbar_face, keeps layer 1's five values in registers and writes
// them once layer 0's cells are updated.  The neighbour's raw sound speed at a
// panel edge is recomputed from its two raw depths rather than stored.
// Registers: the kernel asks for four waves per SIMD (fp64: 128 VGPRs, no
// scratch; five would spill 58 to 114 VGPRs), fp32 runs five.
// 16x16 fp64: 65 360 bytes, under the 64 KiB a launch gets without opting in
// (a plain copy of the tracer layout with eight resident fields: about 66 KB);
// 16x8 fp64: 40 400.
#include "stage_common.h"

namespace {

constexpr int LY_F = 8;      // state fields: (h, M) of two layers
constexpr int LY_NG = 2;     // ghost layers (PLR)

template <int BX, int BY> struct LyGeom {
  static constexpr int NG = LY_NG;
  static constexpr int NX = (BX + 1) * BY, NY = BX * (BY + 1), NE = NX + NY;
  static constexpr int NT = ((NE + 63) / 64) * 64;
  static constexpr int EX = BX + 2 * NG, EY = BY + 2 * NG;
  static constexpr int WS = EX + 1, WF = EY * WS;      // window row / field stride
  static constexpr int BM = BX > BY ? BX : BY, EM = EX > EY ? EX : EY;
  static constexpr int NB = BX + BY + 2;               // normals: x columns, then y rows
  static constexpr int FLR = 5;                        // flux rows: F_h, F_M, cbar_face of one layer
  // window (h, v of both layers, sqrt(g H)) | flux rows | neighbour edge state | neighbour raw cell | normals | lengths
  static constexpr int ELEMS = (LY_F + 1) * WF + FLR * NE + LY_F * 4 * BM + LY_F * 4 * BM + 3 * NB + NE;
  static_assert(EX * EY <= NT, "one window cell per thread");
  static_assert(3 * NB <= NT, "one normal component per thread");
  static_assert(4 * LY_F * EM <= FLR * NE, "the raw strip copy fits in the flux array");
};

template <typename T, int BX, int BY, int LIM, bool REMOTE, bool LIST>
__global__ __launch_bounds__((LyGeom<BX, BY>::NT)) __attribute__((amdgpu_waves_per_eu(4))) void swe_layer_kernel(Args<T> a, const T rr) {
  using G = LyGeom<BX, BY>;
  constexpr int NG = G::NG, FR = LY_F;
  constexpr int NT = G::NT, NX = G::NX, NE = G::NE;
  constexpr int EX = G::EX, EY = G::EY, WS = G::WS, WF = G::WF, BM = G::BM, EM = G::EM;
  extern __shared__ __align__(16) unsigned char ly_smem[];
  T* const s_w = reinterpret_cast<T*>(ly_smem);   // [9][EY][WS]: h_0, v_0 (3), h_1, v_1 (3), sqrt(g H)
  T* const s_fl = s_w + (FR + 1) * WF;            // [5][NE]
  T* const s_pf = s_fl + G::FLR * NE;             // [8][4 BM] neighbour's edge state
  T* const s_pr = s_pf + FR * 4 * BM;             // [8][4 BM] neighbour's raw cell (h, v of both layers)
  T* const s_nrm = s_pr + FR * 4 * BM;            // [3][NB]
  T* const s_len = s_nrm + 3 * G::NB;             // [NE]
  T* const s_raw = s_fl;                          // raw ghosts (until the flux phase): [4][8][EM], layer 0

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
  T xs[4], acs[4], qo[FR];
#pragma unroll
  for (int f = 0; f < 4; ++f) xs[f] = acs[f] = T(0);
#pragma unroll
  for (int f = 0; f < FR; ++f) qo[f] = T(0);
  T iA = T(0), r0 = T(0), r1 = T(0), r2 = T(0);
  T gb[3] = {T(0), T(0), T(0)};
  int pt[4] = {-1, -1, -1, -1};
  if (own) {
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
  // once the window loads are issued
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
    const int r = tid - NIN, rw = r / EX;
    lx = r - rw * EX;
    ly = rw < NG ? rw : EY - 2 * NG + rw;
  } else if (tid - NIN < RING) {
    const int q2 = tid - NIN - 2 * NG * EX, rw = q2 / (2 * NG), c = q2 - rw * (2 * NG);
    ly = NG + rw;
    lx = c < NG ? c : EX - 2 * NG + c;
  }
  if (ly >= 0) {
    const int x = x0 + lx - NG, y = y0 + ly - NG;
    T v[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) v[f] = T(0);
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
        for (int f = 0; f < FR; ++f) v[f] = rp[f];
      } else {
        const long pa = tb + (long)(y + mg) * pw + (x + mg);
#pragma unroll
        for (int f = 0; f < FR; ++f) v[f] = a.Q[(long)f * S + pa];
      }
    }
    if (nrm_i >= 0) s_nrm[nrm_i] = nrm;
    if (edge_ok) s_len[eid] = coef;
    if (own) {
#pragma unroll
      for (int f = 0; f < FR; ++f) qo[f] = v[f];
    }
    const int wi = ly * WS + lx;
    T w[FR];
#pragma unroll
    for (int k = 0; k < 2; ++k) {     // the h = 0 guard of the primitive division, per layer
      const T inv = v[4 * k] != T(0) ? trcp(v[4 * k]) : T(0);
      w[4 * k] = v[4 * k]; w[4 * k + 1] = v[4 * k + 1] * inv; w[4 * k + 2] = v[4 * k + 2] * inv;
      w[4 * k + 3] = v[4 * k + 3] * inv;
    }
#pragma unroll
    for (int f = 0; f < FR; ++f) s_w[f * WF + wi] = w[f];
    s_w[FR * WF + wi] = tsqrt(a.g * tmax(v[0] + v[4], T(0)));
    if (bsides) {   // a raw panel-edge ghost (layer 0) the fix-up interpolates from
      const bool inx = (x >= 0) & (x < n), iny = (y >= 0) & (y < n);
      // strip cells, and the tile-corner cells beyond the strip ends (carried
      // corner ghosts): filed under the side that is a panel edge
      int side = -1, k = 0, al = 0;
      if (!inx) {
        side = x < 0 ? 0 : 1; k = x < 0 ? -1 - x : x - n; al = ly;
        if (!(k < 1 && ((bsides >> side) & 1))) side = -1;
      }
      if (side < 0 && !iny) { side = y < 0 ? 2 : 3; k = y < 0 ? -1 - y : y - n; al = lx; }
      if (side >= 0 && k < 1 && ((bsides >> side) & 1) && !(inx && iny)) {
#pragma unroll
        for (int f = 0; f < FR; ++f) s_raw[(side * FR + f) * EM + al] = w[f];
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
      T* const wf = s_w + f * WF;
      const T* const raw = s_raw + (pside * FR + f) * EM;
      const T g0 = raw[pb - pab], g1 = raw[pb + 1 - pab];
      const T gk = g0 + ptt * (g1 - g0);
      const int co = plow ? 0 : n - 1;
      const T o0 = wf[widx(co, pb)], o1 = wf[widx(co, pb + 1)];
      const T l = o0 + ptt * (o1 - o0);
      const T c = raw[pj - pab];
      const int wend = (pside < 2 ? x0 + BX : y0 + BY) + NG;   // first coordinate past the window
      const T r = wf[widx(plow ? -2 : n + 1, pj)];
      const T nf = c - half_slope<LIM>(c - l, r - c);
      if (plow || n < wend) wf[widx(plow ? -1 : n, pj)] = gk;
      const int pslt = pside * BM + pjl;
      s_pf[f * 4 * BM + pslt] = nf;
      s_pr[f * 4 * BM + pslt] = c;
    }
    __syncthreads();
  }

  // ---- 2. both layers' edge states and fluxes, one edge per thread ---------------
  int pslot = -1;
  bool plo = false;
  if (bsides && edge_ok) {
    if (is_x && ex_ == 0 && (bsides & 1)) { pslot = 0 * BM + ey_ - y0; plo = true; }
    else if (is_x && ex_ == n && (bsides & 2)) { pslot = 1 * BM + ey_ - y0; }
    else if (!is_x && ey_ == 0 && (bsides & 4)) { pslot = 2 * BM + ex_ - x0; plo = true; }
    else if (!is_x && ey_ == n && (bsides & 8)) { pslot = 3 * BM + ex_ - x0; }
  }
  T fl1[5] = {T(0), T(0), T(0), T(0), T(0)};   // layer 1: fluxes and cbar_face, until layer 0 is through
  if (edge_ok) {
    const int cl_ = is_x ? (NG + e_r) * WS + NG - 1 + e_c : (NG - 1 + e_r) * WS + NG + e_c;
    const int cst = is_x ? 1 : WS;
    T sl = s_w[FR * WF + cl_], sr = s_w[FR * WF + cl_ + cst];   // sqrt(g H) of the two cells
    if (pslot >= 0) {   // panel edge: the neighbour's raw cell; its sound speed from its two raw depths
      const T hn = s_pr[0 * 4 * BM + pslot] + s_pr[4 * 4 * BM + pslot];
      if (plo) sl = tsqrt(a.g * tmax(hn, T(0)));
      else sr = tsqrt(a.g * tmax(hn, T(0)));
    }
    const int ni = is_x ? e_c : BX + 1 + e_r;
    const T m0 = s_nrm[ni], m1 = s_nrm[G::NB + ni], m2 = s_nrm[2 * G::NB + ni];
    // one layer at a time (its eight edge-state values live only here): edge
    // states, flux, and the face mean of its depth
    auto layer_flux = [&](int k, T (&fl)[4], T& hbar) {
      T wl[4], wr[4], cl[5], cr[5];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const T* wq = s_w + (4 * k + f) * WF;
        cl[f] = wq[cl_]; cr[f] = wq[cl_ + cst];
        const T q1 = wq[cl_ - cst], p2 = wq[cl_ + 2 * cst];
        const T d1 = cr[f] - cl[f];
        wl[f] = cl[f] + half_slope<LIM>(cl[f] - q1, d1);
        wr[f] = cr[f] - half_slope<LIM>(d1, p2 - cr[f]);
      }
      if (pslot >= 0) {   // panel edge: the neighbour's state and raw cell
        if (plo) {
#pragma unroll
          for (int f = 0; f < 4; ++f) { wl[f] = s_pf[(4 * k + f) * 4 * BM + pslot]; cl[f] = s_pr[(4 * k + f) * 4 * BM + pslot]; }
        } else {
#pragma unroll
          for (int f = 0; f < 4; ++f) { wr[f] = s_pf[(4 * k + f) * 4 * BM + pslot]; cr[f] = s_pr[(4 * k + f) * 4 * BM + pslot]; }
        }
      }
      cl[4] = sl; cr[4] = sr;
      swe_flux<T>(wl, wr, cl, cr, m0, m1, m2, coef, a.g, fl);
      hbar = T(0.5) * (wl[0] + wr[0]);
    };
    T fl0[4], f1[4], hb0, hb1;
    layer_flux(0, fl0, hb0);
    // (the raw strip copy that shared the flux array is dead: the fix-up
    // finished before the barrier above)
#pragma unroll
    for (int f = 0; f < 4; ++f) s_fl[f * NE + eid] = fl0[f];
    layer_flux(1, f1, hb1);
#pragma unroll
    for (int f = 0; f < 4; ++f) fl1[f] = f1[f];
    fl1[4] = rr * hb0;              // c_1 = r h_0 at the face
    s_fl[4 * NE + eid] = hb1;       // c_0 = h_1 at the face
  }
  // the RK operands of the own cell are issued here, not in phase 0: held across
  // the flux phase they cost 32 VGPRs (fp64), which decides the waves per SIMD;
  // their latency hides under the sources and the barriers
  T xs1[4], acs1[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) xs1[f] = acs1[f] = T(0);
  if (own) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (need_x) xs[f] = a.X[(long)f * S + pc];
      if (need_acc) acs[f] = a.acc_in[(long)f * S + pc];
      if (need_x) xs1[f] = a.X[(long)(4 + f) * S + pc];
      if (need_acc) acs1[f] = a.acc_in[(long)(4 + f) * S + pc];
    }
  }
  const int ew = oy * (BX + 1) + ox;            // west x-edge of the cell
  const int es = NX + oy * BX + ox;             // south y-edge
  T Lw = T(0), Le = T(0), Ls = T(0), Ln = T(0);
  if (own) { Lw = s_len[ew]; Le = s_len[ew + 1]; Ls = s_len[es]; Ln = s_len[es + BX]; }
  // own-cell terms of one layer that need no flux: Coriolis, curvature balance
  // g/2 h^2 sum(+-L m)/A (a constant depth is force-free), static topography
  auto base_src = [&](const T* q, T (&src)[3]) {
    const T fc = a.omega2 * r2;
    const T h = q[0];
    const T cor[3] = {r1 * q[3] - r2 * q[2], r2 * q[1] - r0 * q[3], r0 * q[2] - r1 * q[1]};
    const T pb = T(0.5) * a.g * h * h * iA, gh = a.g * h;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const T* nk = s_nrm + k * G::NB;
      const T Sk = Le * nk[ox + 1] - Lw * nk[ox] + Ln * nk[BX + 2 + oy] - Ls * nk[BX + 1 + oy];
      src[k] = -fc * cor[k] + pb * Sk - gh * gb[k];
    }
  };
  auto store = [&](T* base, int f, T v) {
    base[(long)f * S + pc] = v;
  };
  auto store_out = [&](int f, T v) {
    store(a.out, f, v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pt[k] >= 0) a.out[(long)f * S + pt[k]] = v;
  };
  // ---- 3. one layer: divergence + coupling gradient + RK combination + push ------
  // The flux rows hold the layer's F_h, F_M and cbar_face; cc is c_k of the cell.
  auto layer_update = [&](int fo, const T* q, const T* x4, const T* ac4, const T (&src)[3], T cc) {
    T dq[4], o[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const T* fr = s_fl + f * NE;
      dq[f] = -((fr[ew + 1] - fr[ew]) + (fr[es + BX] - fr[es])) * iA;
    }
    // coupling gradient: (cbar_face - c_cell) L m / A over the four faces, tangent part
    const T* cb = s_fl + 4 * NE;
    const T we = (cb[ew + 1] - cc) * Le, ww = (cb[ew] - cc) * Lw, wn = (cb[es + BX] - cc) * Ln, ws = (cb[es] - cc) * Ls;
    T gc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const T* nk = s_nrm + k * G::NB;
      gc[k] = ((we * nk[ox + 1] - ww * nk[ox]) + (wn * nk[BX + 2 + oy] - ws * nk[BX + 1 + oy])) * iA;
    }
    {
      const T d = gc[0] * r0 + gc[1] * r1 + gc[2] * r2;
      gc[0] -= d * r0; gc[1] -= d * r1; gc[2] -= d * r2;
    }
    const T gh = a.g * q[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) dq[1 + k] += src[k] - gh * gc[k];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      T base = T(0);
      if (a.a1 != T(0)) base = a.a1 * q[f];
      if (a.a0 != T(0)) base += a.a0 * x4[f];
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
        for (int f = 0; f < 4; ++f) p[f] += a.c1 * x4[f];
      }
      if (need_acc) {
#pragma unroll
        for (int f = 0; f < 4; ++f) p[f] += a.c0 * ac4[f];
      }
      const T d = p[1] * r0 + p[2] * r1 + p[3] * r2;
      p[1] -= d * r0; p[2] -= d * r1; p[3] -= d * r2;
#pragma unroll
      for (int f = 0; f < 4; ++f) store(a.acc_out, fo + f, p[f]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) store_out(fo + f, o[f]);
  };

  T src[3] = {T(0), T(0), T(0)};
  if (own) base_src(qo, src);
  __syncthreads();
  if (own) layer_update(0, qo, xs, acs, src, qo[4]);
  __syncthreads();              // layer 0's rows are consumed
  if (edge_ok) {
#pragma unroll
    for (int f = 0; f < 5; ++f) s_fl[f * NE + eid] = fl1[f];
  }
  if (own) base_src(qo + 4, src);
  __syncthreads();
  if (own) layer_update(4, qo + 4, xs1, acs1, src, rr * qo[0]);
}

template <typename T, int BX, int BY, int LIM>
int ly_launch_l(const StageDesc* d, hipStream_t s) {
  using G = LyGeom<BX, BY>;
  const Args<T> a = make_args<T>(d);
  const T rr = (T)d->layer_r;
  const size_t lds = (size_t)G::ELEMS * sizeof(T);
  if (lds > 65536) return -13;
  const dim3 grid(d->nblocks), block(G::NT);
  if (d->remote)
    hipLaunchKernelGGL((swe_layer_kernel<T, BX, BY, LIM, true, true>), grid, block, lds, s, a, rr);
  else if (d->blocks)
    hipLaunchKernelGGL((swe_layer_kernel<T, BX, BY, LIM, false, true>), grid, block, lds, s, a, rr);
  else
    hipLaunchKernelGGL((swe_layer_kernel<T, BX, BY, LIM, false, false>), grid, block, lds, s, a, rr);
  return (int)hipGetLastError();
}

template <typename T, int BX, int BY>
int ly_launch_t(const StageDesc* d, hipStream_t s) {
  if (d->nblocks <= 0) return 0;
  if (!(d->layer_r > 0.0 && d->layer_r <= 1.0)) return -17;           // densities increase downwards
  if (d->pw != d->n + 2 * d->mg || d->mg < LY_NG) return -5;
  if (!d->pedge || !d->pe_base || !d->pe_t || d->n < 2) return -12;   // panel-edge tables
  if (!d->mx || !d->my || !d->cgeo || !d->ex || !d->ey) return -6;
  if (!d->push || (d->remote && (!d->gmap || !d->blocks || !d->recv))) return -6;
  if (d->xg) return -10;                                               // no direct xGMI halo
  switch (d->limiter) {
    case 0: return ly_launch_l<T, BX, BY, 0>(d, s);
    case 1: return ly_launch_l<T, BX, BY, 1>(d, s);
    case 2: return ly_launch_l<T, BX, BY, 2>(d, s);
    case 3: return ly_launch_l<T, BX, BY, 3>(d, s);
    case 4: return -11;                                                // PPM: not with layers
  }
  return -7;
}

template <typename T>
int ly_launch_p(int bx, int by, const StageDesc* d, hipStream_t s) {
  if (bx == 16 && by == 16) return ly_launch_t<T, 16, 16>(d, s);
  if (bx == 16 && by == 8) return ly_launch_t<T, 16, 8>(d, s);
  return -2;
}

}  // namespace

extern "C" int stsp_swe_layer_launch(int dtype, int bx, int by, const StageDesc* d, hipStream_t stream) {
  if (dtype == 1) return ly_launch_p<double>(bx, by, d, stream);
  if (dtype == 0) return ly_launch_p<float>(bx, by, d, stream);
  return -4;
}

// dynamic LDS bytes of a launch (host-side contract check)
extern "C" int stsp_swe_layer_lds(int dtype, int bx, int by) {
  const int es = dtype == 1 ? 8 : 4;
  if (bx == 16 && by == 16) return LyGeom<16, 16>::ELEMS * es;
  if (bx == 16 && by == 8) return LyGeom<16, 8>::ELEMS * es;
  return -1;
}
