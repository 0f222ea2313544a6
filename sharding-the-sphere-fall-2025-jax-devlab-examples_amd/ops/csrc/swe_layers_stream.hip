// N-layer (stacked, isopycnal) shallow water, 3 <= L <= 8: one RK stage per
// launch, gfx950 (CDNA4).  models/swe.py::LayeredShallowWater is the twin; two
// layers stay on swe_layer_stage.hip, whose roles, tables, panel-edge fix-up,
// push map, carried corner ghosts, partial blocks and block_sides rule this
// kernel keeps (geometry constants, block decode, block_sides and the window
// cell are block_map.h, the argument check and the launch forms block_stage.h).
// L is a launch value: the state (h_0, M_0, .., h_{L-1}, M_{L-1}) and the
// receive buffer are strided by 4 L.
//
// What differs is how a block walks the stack: it streams the layers through a
// window sized for ONE layer, so its LDS does not depend on L.
//
//   Pass A (column pass, h alone), j = 0 .. L-1: the loader threads bring h_j's
//   window (own cells + two ghost rings, panel-edge treatment of this one
//   field) into window row 0.  Each loader adds its cell into H (ascending j:
//   the order of the twin's sound()); each edge thread reconstructs h_j at its
//   face with the run's limiter and adds m_j = (hL + hR) / 2 into S; each own
//   cell adds h_j into Sc; an edge on a panel edge adds the neighbour's raw
//   depth into the sum its raw sound speed needs.  After the loop the loaders
//   write sqrt(g H) into window row 4.
//
//   Pass B (layer pass), k = 0 .. L-1: layer k's four-field window, primitives,
//   fix-up, edge states and the four fluxes into the shared flux rows, as the
//   two-layer kernel does for one layer.  Then S -= m_k (Sc -= h_k): S is the
//   sum of the layers below, weight 1.  The coupling height is cbar = P + S at
//   the face and c = Pc + Sc in the cell, P the density-weighted sum of the
//   layers above: adjacent layers share one ratio r, rho_j / rho_k = r^(k-j),
//   and P = r (P + m_k) after the layer builds exactly that weight.  Face and
//   cell accumulators go through the same operations in the same order, so
//   uniform layers give cbar - c = 0 exactly, as in the twin; otherwise
//   cbar - c differs from the twin's ascending sum by a few ulp of the total
//   depth, the size of the twin's own rounding.  Layer k's RK combination,
//   stores and ghost pushes follow before the next layer's fluxes.
//
// The accumulators live in registers, not in LDS rows: thread e is edge e and
// thread o is own cell o for the whole launch, and H belongs to the thread that
// loads the window cell, so S, P (edge), Sc, Pc (cell), H (window cell) and the
// neighbour's depth sum are one value each per thread (12 VGPRs in fp64) and
// need no barrier.  LDS then holds one four-primitive window and the sqrt(g H)
// row, five flux rows, the panel-edge rows of one layer (raw strip, neighbour's
// edge state and raw cell), normals and lengths: 16x16 fp64 50 384 bytes,
// 16x8 fp64 30 800 (the two-layer kernel: 65 360 / 40 400).  The raw strip has
// rows of its own (it does not share the flux rows), so layer k + 1's window
// load needs no barrier after layer k's update: three barriers per layer in
// pass B (four at a panel edge), two in pass A (three).
// Registers: the layer loop keeps the own cell's geometry, the push targets and
// the accumulators live across the flux phase, so fp64 wants 154 to 158 VGPRs
// and spills 124 to 136 bytes at the 128 of four waves per SIMD: the kernel asks
// for three (no scratch).  A 16x16 block is nine waves, one block per CU either
// way; 16x8 runs two blocks per CU rather than three.  fp32: 104 to 105, four.
// Known cost: every h_j is read twice per stage.  Pass A prefetches h_{j+1}
// under layer j's barriers.
#include "block_stage.h"

namespace {

constexpr int LS_NG = 2;       // ghost layers (PLR)
constexpr int LS_MIN = 3, LS_MAX = 8;

template <int BX, int BY> struct LsGeom : BlockGeom<BX, BY, LS_NG> {
  using B = BlockGeom<BX, BY, LS_NG>;
  using B::WF; using B::NE; using B::BM; using B::NB; using B::EM; using B::FLR;   // FLR: F_h, F_M, cbar_face of one layer
  // window (h, v of one layer, sqrt(g H)) | flux rows | neighbour edge state | neighbour raw cell | raw strips |
  // normals | lengths
  static constexpr int ELEMS = 5 * WF + FLR * NE + 4 * 4 * BM + 4 * 4 * BM + 4 * 4 * EM + 3 * NB + NE;
};

template <typename T, int BX, int BY, int LIM, bool REMOTE, bool LIST>
__global__ __launch_bounds__((LsGeom<BX, BY>::NT)) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 8 ? 3 : 4))) void swe_layers_stream_kernel(
    Args<T> a, const T rr, const int nl) {
  using G = LsGeom<BX, BY>;
  constexpr int NG = G::NG;
  constexpr int NT = G::NT, NX = G::NX, NE = G::NE;
  constexpr int EX = G::EX, EY = G::EY, WS = G::WS, WF = G::WF, BM = G::BM, EM = G::EM;
  extern __shared__ __align__(16) unsigned char ls_smem[];
  T* const s_w = reinterpret_cast<T*>(ls_smem);   // [5][EY][WS]: h, v (3) of the layer in flight, sqrt(g H)
  T* const s_fl = s_w + 5 * WF;                   // [5][NE]
  T* const s_pf = s_fl + G::FLR * NE;             // [4][4 BM] neighbour's edge state
  T* const s_pr = s_pf + 4 * 4 * BM;              // [4][4 BM] neighbour's raw cell (h, v)
  T* const s_raw = s_pr + 4 * 4 * BM;             // [4 sides][4][EM] raw ghosts, layer 0 of the strip
  T* const s_nrm = s_raw + 4 * 4 * EM;            // [3][NB]
  T* const s_len = s_nrm + 3 * G::NB;             // [NE]

  const int bid = LIST ? a.blocks[blockIdx.x] : xcd_remap(blockIdx.x, a.nblocks);
  const int n = a.n, S = a.S, nn = n * n, mg = a.mg, pw = a.pw;
  const int FR = 4 * nl;                          // fields of the state and of a receive-buffer row
  const BlockPos bp = G::decode(bid, n);
  const int tile = bp.tile, x0 = bp.x0, y0 = bp.y0;
  const int tid = threadIdx.x;
  const long tb = (long)tile * pw * pw;
  const int gbase = tile * nn;
  const int pe_word = a.pedge[tile];
  const int bsides = G::block_sides(pe_word, x0, y0, n);

  // ---- 0. own cell operands ---------------------------------------------------
  const int ox = tid % BX, oy = tid / BX;
  const int cx = x0 + ox, cy = y0 + oy;
  const bool own = tid < BX * BY && cx < n && cy < n;
  const long pc = tb + (long)(cy + mg) * pw + (cx + mg);
  const bool need_x = (a.a0 != T(0)) || (a.acc_out && a.c1 != T(0));
  const bool need_acc = a.acc_out && a.acc_in && (a.c0 != T(0));
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
  // edge normals of this block's columns / rows
  if (tid < 3 * (BX + 1)) {
    const int k = tid / (BX + 1), c = tid - k * (BX + 1);
    s_nrm[k * G::NB + c] = x0 + c <= n ? a.mx[(tile * 3 + k) * (n + 1) + x0 + c] : T(0);
  } else if (tid < 3 * G::NB) {
    const int u = tid - 3 * (BX + 1);
    const int k = u / (BY + 1), c = u - k * (BY + 1);
    s_nrm[k * G::NB + BX + 1 + c] = y0 + c <= n ? a.my[(tile * 3 + k) * (n + 1) + y0 + c] : T(0);
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
  if (edge_ok) {
    coef = is_x ? a.ex[(long)tile * n * (n + 1) + ey_ * (n + 1) + ex_] : a.ey[(long)tile * (n + 1) * n + ey_ * n + ex_];
    s_len[eid] = coef;
  }
  int pslot = -1;
  bool plo = false;
  if (bsides && edge_ok) {
    if (is_x && ex_ == 0 && (bsides & 1)) { pslot = 0 * BM + ey_ - y0; plo = true; }
    else if (is_x && ex_ == n && (bsides & 2)) { pslot = 1 * BM + ey_ - y0; }
    else if (!is_x && ey_ == 0 && (bsides & 4)) { pslot = 2 * BM + ex_ - x0; plo = true; }
    else if (!is_x && ey_ == n && (bsides & 8)) { pslot = 3 * BM + ex_ - x0; }
  }
  const int cl_ = is_x ? (NG + e_r) * WS + NG - 1 + e_c : (NG - 1 + e_r) * WS + NG + e_c;   // left cell of the edge
  const int cst = is_x ? 1 : WS;

  // ---- 1. this thread's window cell: where every layer's values come from --------
  // Thread o < BX BY loads its own cell, the next threads one cell each of
  // the two-cell ring around the block: NG rows below and above, then NG
  // columns left and right.  Field f of the state is lp[lbase + f * lstr].
  int ly, lx;
  G::window_cell(tid, ly, lx);
  const int wi = ly * WS + lx;
  const T* lp = nullptr;           // null: no window cell, or one past a partial block (zeros)
  long lbase = 0, lstr = 0;
  int raw_i = -1;                  // row of s_raw (field 0) this cell is filed under
  if (ly >= 0) {
    const int x = x0 + lx - NG, y = y0 + ly - NG;
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
      if (m < 0) { lp = a.recv; lbase = (long)(-1 - m) * FR; lstr = 1; }
      else { lp = a.Q; lbase = tb + (long)(y + mg) * pw + (x + mg); lstr = S; }
    }
    if (bsides) {   // a raw panel-edge ghost (layer 0 of the strip) the fix-up interpolates from
      const bool inx = (x >= 0) & (x < n), iny = (y >= 0) & (y < n);
      // strip cells, and the tile-corner cells beyond the strip ends (carried
      // corner ghosts): filed under the side that is a panel edge
      int side = -1, k = 0, al = 0;
      if (!inx) {
        side = x < 0 ? 0 : 1; k = x < 0 ? -1 - x : x - n; al = ly;
        if (!(k < 1 && ((bsides >> side) & 1))) side = -1;
      }
      if (side < 0 && !iny) { side = y < 0 ? 2 : 3; k = y < 0 ? -1 - y : y - n; al = lx; }
      if (side >= 0 && k < 1 && ((bsides >> side) & 1) && !(inx && iny)) raw_i = side * 4 * EM + al;
    }
  }

  // panel edges: interpolated ghosts + the neighbour's edge state and raw cell of
  // the first nf window rows (models/base.py::reconstruct; the block-wide form
  // of stage_kernel.hip 1a).  Block-uniform; ends with a barrier.
  auto fixup = [&](int nf) {
    for (int u = tid; u < nf * 4 * BM; u += NT) {
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
      const T* const raw = s_raw + (pside * 4 + f) * EM;
      const T g0 = raw[pb - pab], g1 = raw[pb + 1 - pab];
      const T gk = g0 + ptt * (g1 - g0);
      const int co = plow ? 0 : n - 1;
      const T o0 = wf[widx(co, pb)], o1 = wf[widx(co, pb + 1)];
      const T l = o0 + ptt * (o1 - o0);
      const T c = raw[pj - pab];
      const int wend = (pside < 2 ? x0 + BX : y0 + BY) + NG;   // first coordinate past the window
      const T r = wf[widx(plow ? -2 : n + 1, pj)];
      const T nf_ = c - half_slope<LIM>(c - l, r - c);
      if (plow || n < wend) wf[widx(plow ? -1 : n, pj)] = gk;
      const int pslt = pside * BM + pjl;
      s_pf[f * 4 * BM + pslt] = nf_;
      s_pr[f * 4 * BM + pslt] = c;
    }
    __syncthreads();
  };

  // ---- 2. pass A: the column sums -----------------------------------------------
  T Hs = T(0);                    // window cell: sum of the depths (sound speed)
  T Sf = T(0), Pf = T(0);         // edge: depths below (weight 1) / above (density-weighted) at the face
  T Sc = T(0), Pc = T(0);         // own cell: the same of the cell averages
  T hnb = T(0);                   // panel edge: the neighbour's raw depths
  T hv = lp ? lp[lbase] : T(0);
  for (int j = 0; j < nl; ++j) {
    if (ly >= 0) {
      s_w[wi] = hv;
      if (raw_i >= 0) s_raw[raw_i] = hv;
      Hs += hv;
      if (own) Sc += hv;
    }
    const T hnext = (lp && j + 1 < nl) ? lp[lbase + (long)(4 * (j + 1)) * lstr] : T(0);
    __syncthreads();
    if (bsides) fixup(1);
    if (edge_ok) {
      const T cl = s_w[cl_], cr = s_w[cl_ + cst];
      const T q1 = s_w[cl_ - cst], p2 = s_w[cl_ + 2 * cst];
      const T d1 = cr - cl;
      T wl = cl + half_slope<LIM>(cl - q1, d1);
      T wr = cr - half_slope<LIM>(d1, p2 - cr);
      if (pslot >= 0) {
        if (plo) wl = s_pf[pslot]; else wr = s_pf[pslot];
        hnb += s_pr[pslot];
      }
      const T mj = T(0.5) * (wl + wr);
      Sf += mj;
    }
    __syncthreads();              // the window row is free for h_{j+1}
    hv = hnext;
  }
  if (ly >= 0) s_w[4 * WF + wi] = tsqrt(a.g * tmax(Hs, T(0)));
  const T snb = tsqrt(a.g * tmax(hnb, T(0)));   // the neighbour's raw sound speed at a panel edge

  // ---- 3. pass B: one layer at a time through the window --------------------------
  const int ew = G::west_edge(ox, oy);           // west x-edge of the cell
  const int es = G::south_edge(ox, oy);          // south y-edge
  const int ni = is_x ? e_c : BX + 1 + e_r;
  for (int k = 0; k < nl; ++k) {
    const int fo = 4 * k;
    // 3a. layer k's window -> LDS as primitives
    T qo[4] = {T(0), T(0), T(0), T(0)};
    if (ly >= 0) {
      T v[4] = {T(0), T(0), T(0), T(0)};
      if (lp) {
#pragma unroll
        for (int f = 0; f < 4; ++f) v[f] = lp[lbase + (long)(fo + f) * lstr];
      }
      if (own) {
#pragma unroll
        for (int f = 0; f < 4; ++f) qo[f] = v[f];
      }
      const T inv = v[0] != T(0) ? trcp(v[0]) : T(0);     // the h = 0 guard of the primitive division
      const T w[4] = {v[0], v[1] * inv, v[2] * inv, v[3] * inv};
#pragma unroll
      for (int f = 0; f < 4; ++f) s_w[f * WF + wi] = w[f];
      if (raw_i >= 0) {
#pragma unroll
        for (int f = 0; f < 4; ++f) s_raw[raw_i + f * EM] = w[f];
      }
    }
    __syncthreads();
    if (bsides) fixup(4);
    // 3b. edge states, flux and the coupling height at the face, one edge per thread
    if (edge_ok) {
      T sl = s_w[4 * WF + cl_], sr = s_w[4 * WF + cl_ + cst];   // sqrt(g H) of the two cells
      if (pslot >= 0) { if (plo) sl = snb; else sr = snb; }
      const T m0 = s_nrm[ni], m1 = s_nrm[G::NB + ni], m2 = s_nrm[2 * G::NB + ni];
      T wl[4], wr[4], cl[5], cr[5], fl[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const T* wq = s_w + f * WF;
        cl[f] = wq[cl_]; cr[f] = wq[cl_ + cst];
        const T q1 = wq[cl_ - cst], p2 = wq[cl_ + 2 * cst];
        const T d1 = cr[f] - cl[f];
        wl[f] = cl[f] + half_slope<LIM>(cl[f] - q1, d1);
        wr[f] = cr[f] - half_slope<LIM>(d1, p2 - cr[f]);
      }
      if (pslot >= 0) {   // panel edge: the neighbour's state and raw cell
        if (plo) {
#pragma unroll
          for (int f = 0; f < 4; ++f) { wl[f] = s_pf[f * 4 * BM + pslot]; cl[f] = s_pr[f * 4 * BM + pslot]; }
        } else {
#pragma unroll
          for (int f = 0; f < 4; ++f) { wr[f] = s_pf[f * 4 * BM + pslot]; cr[f] = s_pr[f * 4 * BM + pslot]; }
        }
      }
      cl[4] = sl; cr[4] = sr;
      swe_flux<T>(wl, wr, cl, cr, m0, m1, m2, coef, a.g, fl);
#pragma unroll
      for (int f = 0; f < 4; ++f) s_fl[f * NE + eid] = fl[f];
      const T mk = T(0.5) * (wl[0] + wr[0]);     // pass A's m_k: the same operations on the same values
      Sf -= mk;
      s_fl[4 * NE + eid] = Pf + Sf;
      Pf = rr * (Pf + mk);
    }
    // the RK operands of the own cell are issued here, not with the window: held
    // across the flux phase they cost 32 VGPRs (fp64) and the kernel spills
    T xs[4] = {T(0), T(0), T(0), T(0)}, acs[4] = {T(0), T(0), T(0), T(0)};
    if (own) {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if (need_x) xs[f] = a.X[(long)(fo + f) * S + pc];
        if (need_acc) acs[f] = a.acc_in[(long)(fo + f) * S + pc];
      }
    }
    __syncthreads();
    // 3c. own cell: divergence + sources + coupling gradient + RK combination + push
    if (own) {
      const T h = qo[0];
      const T Lw = s_len[ew], Le = s_len[ew + 1], Ls = s_len[es], Ln = s_len[es + BX];
      Sc -= h;
      const T cc = Pc + Sc;
      Pc = rr * (Pc + h);
      // Coriolis, curvature balance g/2 h^2 sum(+-L m)/A (a constant depth is
      // force-free), static topography
      const T fc = a.omega2 * r2;
      const T cor[3] = {r1 * qo[3] - r2 * qo[2], r2 * qo[1] - r0 * qo[3], r0 * qo[2] - r1 * qo[1]};
      const T pb = T(0.5) * a.g * h * h * iA, gh = a.g * h;
      T dq[4], o[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const T* fr = s_fl + f * NE;
        dq[f] = -((fr[ew + 1] - fr[ew]) + (fr[es + BX] - fr[es])) * iA;
      }
      // coupling gradient: (cbar_face - c_cell) L m / A over the four faces, tangent part
      const T* cb = s_fl + 4 * NE;
      const T we = (cb[ew + 1] - cc) * Le, ww = (cb[ew] - cc) * Lw, wn = (cb[es + BX] - cc) * Ln, ws = (cb[es] - cc) * Ls;
      T gc[3], src[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const T* nk = s_nrm + c * G::NB;
        const T Sk = Le * nk[ox + 1] - Lw * nk[ox] + Ln * nk[BX + 2 + oy] - Ls * nk[BX + 1 + oy];
        src[c] = -fc * cor[c] + pb * Sk - gh * gb[c];
        gc[c] = ((we * nk[ox + 1] - ww * nk[ox]) + (wn * nk[BX + 2 + oy] - ws * nk[BX + 1 + oy])) * iA;
      }
      {
        const T d = gc[0] * r0 + gc[1] * r1 + gc[2] * r2;
        gc[0] -= d * r0; gc[1] -= d * r1; gc[2] -= d * r2;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) dq[1 + c] += src[c] - gh * gc[c];
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
        for (int f = 0; f < 4; ++f) a.acc_out[(long)(fo + f) * S + pc] = p[f];
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        a.out[(long)(fo + f) * S + pc] = o[f];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (pt[q] >= 0) a.out[(long)(fo + f) * S + pt[q]] = o[f];
      }
    }
    // no barrier here: layer k + 1 writes the window (its readers passed the
    // barrier before 3c) and the raw strips (read before the barrier of 3b);
    // the flux rows are written only after the next barrier
  }
}

template <typename T, int BX, int BY, int LIM>
int ls_launch_l(const StageDesc* d, hipStream_t s) {
  using G = LsGeom<BX, BY>;
  const Args<T> a = make_args<T>(d);
  const T rr = (T)d->layer_r;
  const size_t lds = (size_t)G::ELEMS * sizeof(T);
  return block_launch(d, swe_layers_stream_kernel<T, BX, BY, LIM, true, true>, swe_layers_stream_kernel<T, BX, BY, LIM, false, true>, swe_layers_stream_kernel<T, BX, BY, LIM, false, false>, G::NT, lds, s, a, rr, (int)d->layers);
}

template <typename T, int BX, int BY>
int ls_launch_t(const StageDesc* d, hipStream_t s) {
  if (d->nblocks <= 0) return 0;
  if (d->layers < LS_MIN || d->layers > LS_MAX) return -18;            // two layers: swe_layer_stage.hip
  if (!(d->layer_r > 0.0 && d->layer_r <= 1.0)) return -17;           // densities increase downwards
  if (const int rc = block_args_check(d, LS_NG)) return rc;
  switch (d->limiter) {
    case 0: return ls_launch_l<T, BX, BY, 0>(d, s);
    case 1: return ls_launch_l<T, BX, BY, 1>(d, s);
    case 2: return ls_launch_l<T, BX, BY, 2>(d, s);
    case 3: return ls_launch_l<T, BX, BY, 3>(d, s);
    case 4: return -11;                                                // PPM: not with layers
  }
  return -7;
}

template <typename T>
int ls_launch_p(int bx, int by, const StageDesc* d, hipStream_t s) {
  if (bx == 16 && by == 16) return ls_launch_t<T, 16, 16>(d, s);
  if (bx == 16 && by == 8) return ls_launch_t<T, 16, 8>(d, s);
  return -2;
}

}  // namespace

extern "C" int stsp_swe_layers_stream_launch(int dtype, int bx, int by, const StageDesc* d, hipStream_t stream) {
  if (dtype == 1) return ls_launch_p<double>(bx, by, d, stream);
  if (dtype == 0) return ls_launch_p<float>(bx, by, d, stream);
  return -4;
}

// dynamic LDS bytes of a launch, the same for every L (host-side contract check)
extern "C" int stsp_swe_layers_stream_lds(int dtype, int bx, int by) {
  const int es = dtype == 1 ? 8 : 4;
  if (bx == 16 && by == 16) return LsGeom<16, 16>::ELEMS * es;
  if (bx == 16 && by == 8) return LsGeom<16, 8>::ELEMS * es;
  return -1;
}
