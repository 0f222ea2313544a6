// Integer maps of the plain block stage kernels (swe_tracer_stage.hip,
// swe_layer_stage.hip, swe_layers_stream.hip): the block's geometry constants,
// which block a launch index is, which of its sides lie on a cube edge, and
// which window cell a thread loads.  Pure functions of integers, so a plain
// host compiler can include this header (tests/block_map_check.cpp checks every
// map against a brute-force loop).
//
// A block of BX x BY cells at (x0, y0) of an n x n tile works on a window of
// EX x EY cells (the block and NG ghost layers around it).  Thread e is edge e
// (x-edges, then y-edges), thread o < BX BY loads and updates own cell o, the
// next threads load one cell each of the ring around the block.  Bit s of a
// side word stands for side s: 0: x < 0, 1: x >= n, 2: y < 0, 3: y >= n.
//
// Only maps that leave the compiled kernels as they were live here.  The edge
// decode, the push indices, the ghost-table lookup and the raw-strip filing
// changed the kernels' registers and cost 1 to 2 % when they were moved, and
// stay in the kernels (profiles/block_stage).
#pragma once

#ifdef __HIPCC__
#define BM_HD __host__ __device__ __forceinline__
#else
#define BM_HD inline
#endif

struct BlockPos { int tile, x0, y0; };

template <int BX_, int BY_, int NG_> struct BlockGeom {
  static constexpr int BX = BX_, BY = BY_, NG = NG_;
  static constexpr int NX = (BX + 1) * BY, NY = BX * (BY + 1), NE = NX + NY;
  static constexpr int NT = ((NE + 63) / 64) * 64;
  static constexpr int EX = BX + 2 * NG, EY = BY + 2 * NG;
  static constexpr int WS = EX + 1, WF = EY * WS;      // window row / field stride
  static constexpr int BM = BX > BY ? BX : BY, EM = EX > EY ? EX : EY;
  static constexpr int NB = BX + BY + 2;               // normals: x columns, then y rows
  static constexpr int FLR = 5;                        // flux rows
  static_assert(EX * EY <= NT, "one window cell per thread");
  static_assert(3 * NB <= NT, "one normal component per thread");

  BM_HD static BlockPos decode(int bid, int n) {
    const int nbx = (n + BX - 1) / BX, nby = (n + BY - 1) / BY;
    const int tile = bid / (nbx * nby);
    const int rem = bid - tile * nbx * nby;
    const int yb = rem / nbx, xb = rem - yb * nbx;
    return {tile, xb * BX, yb * BY};
  }

  // sides of this block on a cube edge: a side counts as soon as the window
  // reaches its ghost strip (the last block may be one cell wide)
  BM_HD static int block_sides(int pe_word, int x0, int y0, int n) {
    return (x0 == 0 ? (pe_word & 1) : 0) | (x0 + BX + NG > n ? (pe_word & 2) : 0) |
           (y0 == 0 ? (pe_word & 4) : 0) | (y0 + BY + NG > n ? (pe_word & 8) : 0);
  }

  // Window cell (ly, lx) of a thread, ly = -1: none.  Thread o < BX BY has its
  // own cell, the next RING threads one cell each of the ring around the
  // block: NG rows below and above, then NG columns left and right.
  BM_HD static void window_cell(int tid, int& ly, int& lx) {
    constexpr int NIN = BX * BY, RING = EX * EY - NIN;
    ly = -1; lx = 0;
    if (tid < NIN) {
      ly = NG + tid / BX; lx = NG + tid % BX;
    } else if (tid - NIN < 2 * NG * EX) {
      const int r = tid - NIN, rw = r / EX;
      lx = r - rw * EX;
      ly = rw < NG ? rw : EY - 2 * NG + rw;
    } else if (tid - NIN < RING) {
      const int q2 = tid - NIN - 2 * NG * EX, rw = q2 / (2 * NG), c = q2 - rw * (2 * NG);
      ly = NG + rw;
      lx = c < NG ? c : EX - 2 * NG + c;
    }
  }

  // west x-edge and south y-edge of own cell (ox, oy); east is west + 1, north south + BX
  BM_HD static int west_edge(int ox, int oy) { return oy * (BX + 1) + ox; }
  BM_HD static int south_edge(int ox, int oy) { return NX + oy * BX + ox; }
};
