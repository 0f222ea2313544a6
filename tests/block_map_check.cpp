// Host check of the integer maps of the block stage kernels
// (ops/csrc/block_map.h), built and run by tests/test_block_map.py as plain
// C++: every map against a brute-force loop over the block's window and edges,
// for both block shapes, two and three ghost layers, tile sizes around the
// block size, every block of the tile and every panel-edge word.
#include <cstdio>
#include <vector>

#include "block_map.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (failures++ < 20) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                      \
  } while (0)

const int SIZES[] = {2, 3, 15, 16, 17, 18, 20, 31, 32, 33, 34};

// every window cell has exactly one thread, own cell o is thread o, and the
// own cell's west / south edges are the ids the edge numbering gives them
template <int BX, int BY, int NG> void check_window() {
  using G = BlockGeom<BX, BY, NG>;
  std::vector<int> seen(G::EX * G::EY, 0);
  for (int tid = 0; tid < G::NT; ++tid) {
    int ly, lx;
    G::window_cell(tid, ly, lx);
    if (ly < 0) continue;
    CHECK(ly < G::EY && lx >= 0 && lx < G::EX, "tid %d -> (%d, %d)", tid, ly, lx);
    if (!(ly < G::EY && lx >= 0 && lx < G::EX)) continue;
    seen[ly * G::EX + lx]++;
    const bool inner = ly >= NG && ly < NG + BY && lx >= NG && lx < NG + BX;
    CHECK(inner == (tid < BX * BY), "tid %d", tid);
    if (tid < BX * BY) CHECK(ly == NG + tid / BX && lx == NG + tid % BX, "own cell %d -> (%d, %d)", tid, ly, lx);
  }
  for (int i = 0; i < G::EX * G::EY; ++i) CHECK(seen[i] == 1, "window cell %d has %d threads", i, seen[i]);
  // x-edges are numbered row by row (BX + 1 a row), then the y-edges (BX a row)
  int id = 0;
  std::vector<int> xe((BX + 1) * BY), ye(BX * (BY + 1));
  for (int r = 0; r < BY; ++r)
    for (int c = 0; c <= BX; ++c) xe[r * (BX + 1) + c] = id++;
  for (int r = 0; r <= BY; ++r)
    for (int c = 0; c < BX; ++c) ye[r * BX + c] = id++;
  CHECK(id == G::NE && G::NE <= G::NT, "%d edges", id);
  for (int oy = 0; oy < BY; ++oy)
    for (int ox = 0; ox < BX; ++ox) {
      CHECK(G::west_edge(ox, oy) == xe[oy * (BX + 1) + ox] && G::west_edge(ox, oy) + 1 == xe[oy * (BX + 1) + ox + 1], "cell (%d, %d)", ox, oy);
      CHECK(G::south_edge(ox, oy) == ye[oy * BX + ox] && G::south_edge(ox, oy) + BX == ye[(oy + 1) * BX + ox], "cell (%d, %d)", ox, oy);
    }
}

template <int BX, int BY, int NG> void check_block(int n, int tile, int xb, int yb) {
  using G = BlockGeom<BX, BY, NG>;
  const int nbx = (n + BX - 1) / BX, nby = (n + BY - 1) / BY;
  const BlockPos bp = G::decode((tile * nby + yb) * nbx + xb, n);
  CHECK(bp.tile == tile && bp.x0 == xb * BX && bp.y0 == yb * BY, "n %d block (%d, %d, %d)", n, tile, xb, yb);
  const int x0 = xb * BX, y0 = yb * BY;
  for (int w = 0; w < 16; ++w) {
    // block_sides: the word's bit and a window cell in the side's ghost strip
    // (n = 17, 33: the one-cell-wide last block; 18, 34: the two-cell-wide one)
    int want = 0;
    for (int ly = 0; ly < G::EY; ++ly)
      for (int lx = 0; lx < G::EX; ++lx) {
        const int x = x0 + lx - NG, y = y0 + ly - NG;
        const bool inx = x >= 0 && x < n, iny = y >= 0 && y < n;
        if (iny && x < 0) want |= w & 1;
        if (iny && x >= n && x < n + NG) want |= w & 2;
        if (inx && y < 0) want |= w & 4;
        if (inx && y >= n && y < n + NG) want |= w & 8;
      }
    const int bs = G::block_sides(w, x0, y0, n);
    CHECK(bs == want, "n %d block (%d, %d) word %d: %d, want %d", n, x0, y0, w, bs, want);
  }
}

template <int BX, int BY, int NG> void check_geom() {
  check_window<BX, BY, NG>();
  for (int n : SIZES)
    for (int tile : {0, 5})
      for (int yb = 0; yb < (n + BY - 1) / BY; ++yb)
        for (int xb = 0; xb < (n + BX - 1) / BX; ++xb) check_block<BX, BY, NG>(n, tile, xb, yb);
}

}  // namespace

int main() {
  check_geom<16, 16, 2>();
  check_geom<16, 16, 3>();
  check_geom<16, 8, 2>();
  check_geom<16, 8, 3>();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("block maps ok\n");
  return 0;
}
