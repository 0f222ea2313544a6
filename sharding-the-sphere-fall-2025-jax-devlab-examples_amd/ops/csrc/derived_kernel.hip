// Derived shallow-water fields on the device: relative vorticity, divergence,
// potential vorticity and the invariants of the running state (mass, energy,
// potential enstrophy, circulation, |circulation|, Courant maximum).  The
// definitions are those of models/derived.py, the PyTorch twin.
//
// One workgroup per 16 x 16 cell block of a tile (ragged at the tile end), 256
// threads, two phases:
//
//  load     every thread loads its own cell (h, M) from the padded state and
//           stores v = M / h to the LDS window; threads 0..63 then fill the four
//           ring strips.  A ring cell inside the tile is another interior cell; one
//           outside comes through gmap (remote: recv), never from the padded
//           state's ghost slots, which are not current after a fused launch.  On a
//           panel-edge side the thread evaluates the layer-0 interpolation pair
//           (pe_base, pe_t) directly from its two source cells; along-strip
//           positions -1 and n are the carried corner ghosts (cgmap).  The block's
//           four corner cells are never read by the 5-point stencil and stay unset.
//  compute  one thread per cell: 4 edge averages, 4 chord and 4 normal dot
//           products, zeta, delta, q; coalesced row stores to fields [3][T][n][n].
//
// LDS window: three components, 18 rows of WS = 48 values.  A half-wave (the
// banking group of ds_read_b64 / ds_read_b32) is two block rows of 16 lanes; its
// two 16-value spans fall on disjoint banks iff the row stride is 16 mod 32
// values (fp64: 2 WS = 32 mod 64 dwords; fp32: WS = 16 mod 32 dwords), for the
// row-pair (y-edge) and the column-pair (x-edge) reads alike, since a column
// shift moves both spans together.  18 (stride = window width) would overlap the
// spans by two values: a 2-way conflict on every read.
//
// Invariants: fp64 accumulators whatever the state type; a fixed shuffle tree
// inside each wave, the four waves folded in wave order through LDS, one record
// of 8 doubles per block (plain stores, no atomics); a second one-workgroup
// launch folds the records in block order with a fixed association (32 contiguous
// chunks, then the chunks in order).  The result does not depend on how blocks
// are scheduled and repeats bit for bit.  No polling, nothing persistent.
//
// Contraction is off in this file: every product and sum rounds on its own, in
// the association the twin writes down, so the fields differ from the twin's only
// where a division or a square root does.  The kernel is bound by its table and
// state reads, not by the multiply-adds.
#include "stsp_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int DB = 16;          // block edge
constexpr int WW = DB + 2;      // window edge
constexpr int WS = 48;          // window row stride (16 mod 32: see above)
constexpr int NREC = 8;         // record: 5 sums, 1 max, 2 spare
constexpr int FOLD_CHUNKS = 32;

template <typename T>
struct DArgs {
  const T* Q;
  const T* recv;
  const int* gmap;
  const int* cgmap;
  const int* pedge;
  const int* pe_base;
  const T* pe_t;
  const T* cdx;
  const T* cdy;
  const T* mx;
  const T* my;
  const T* ex;
  const T* ey;
  const T* invA;
  const T* area;
  const T* idxy;
  const T* b;
  const T* rz;
  T* fields;
  double* partials;
  int ntile, n, S, mg, pw, nbx, nby;
  T g, omega2;
};

// max that keeps a NaN (as torch.max does)
__device__ __forceinline__ double nanmax(double a, double b) { return (a > b || a != a) ? a : b; }

template <typename T>
struct V3 {
  T x, y, z;
};

// v = M / h of the cell behind ghost-map code c (>= 0: padded offset, < 0: receive slot -1 - c)
template <typename T>
__device__ __forceinline__ V3<T> load_v(const DArgs<T>& a, int c) {
  T h, m0, m1, m2;
  if (c >= 0) {
    h = a.Q[c];
    m0 = a.Q[(size_t)a.S + c];
    m1 = a.Q[2 * (size_t)a.S + c];
    m2 = a.Q[3 * (size_t)a.S + c];
  } else {
    const T* r = a.recv + 4 * (size_t)(-1 - c);
    h = r[0];
    m0 = r[1];
    m1 = r[2];
    m2 = r[3];
  }
  const T s = h != T(0) ? h : T(1);
  return {m0 / s, m1 / s, m2 / s};
}

// ghost-map code of layer-0 strip position p in [-1, n] of tile t, side s (W, E, S, N)
template <typename T>
__device__ __forceinline__ int strip_code(const DArgs<T>& a, int t, int s, int p) {
  if (p >= 0 && p < a.n) return a.gmap[((size_t)(t * 4 + s) * a.mg) * a.n + p];
  // strip end: the corner ghost (quad = (x side E) | 2 (y side N), a = b = 0)
  const int hi = p >= a.n;
  const int quad = s < 2 ? ((s & 1) | (hi << 1)) : (hi | ((s & 1) << 1));
  return a.cgmap[(size_t)(t * 4 + quad) * a.mg * a.mg];
}

template <typename T>
__global__ __launch_bounds__(256) void derived_kernel(const DArgs<T> a) {
  __shared__ T win[3][WW * WS];
  __shared__ double red[4][NREC];
  const int tid = threadIdx.x;
  const int n = a.n, pw = a.pw, mg = a.mg;
  int blk = blockIdx.x;
  const int xb = blk % a.nbx;
  blk /= a.nbx;
  const int yb = blk % a.nby;
  const int t = blk / a.nby;
  const int x0 = xb * DB, y0 = yb * DB;
  const int bw = min(DB, n - x0), bh = min(DB, n - y0);
  const int lx = tid & (DB - 1), ly = tid >> 4;
  const bool own = lx < bw && ly < bh;
  const int x = x0 + lx, y = y0 + ly;

  // ---- load: own cell ----------------------------------------------------------
  T h = T(1), m0 = T(0), m1 = T(0), m2 = T(0);
  V3<T> v = {T(0), T(0), T(0)};
  if (own) {
    const size_t c = ((size_t)t * pw + y + mg) * pw + x + mg;
    h = a.Q[c];
    m0 = a.Q[(size_t)a.S + c];
    m1 = a.Q[2 * (size_t)a.S + c];
    m2 = a.Q[3 * (size_t)a.S + c];
    const T s = h != T(0) ? h : T(1);
    v = {m0 / s, m1 / s, m2 / s};
    const int w = (ly + 1) * WS + lx + 1;
    win[0][w] = v.x;
    win[1][w] = v.y;
    win[2][w] = v.z;
  }
  // ---- load: ring strips (S, N, W, E of the block), 16 threads each -------------
  if (tid < 4 * DB) {
    const int rs = tid >> 4, p = tid & (DB - 1);
    const bool horiz = rs < 2;                 // S / N strip: runs along x
    if (p < (horiz ? bw : bh)) {
      const int wx = horiz ? p : (rs == 2 ? -1 : bw);
      const int wy = horiz ? (rs == 0 ? -1 : bh) : p;
      const int gx = x0 + wx, gy = y0 + wy;    // tile coordinates, one of them may be -1 or n
      V3<T> r;
      if (gx >= 0 && gx < n && gy >= 0 && gy < n) {
        r = load_v(a, (int)(((size_t)t * pw + gy + mg) * pw + gx + mg));
      } else {
        const int side = gx < 0 ? 0 : (gx >= n ? 1 : (gy < 0 ? 2 : 3));
        const int pos = side < 2 ? gy : gx;
        if ((a.pedge[t] >> side) & 1) {
          const size_t k = ((size_t)(t * 4 + side) * 3) * n + pos;
          const int b = a.pe_base[k];
          const T tt = a.pe_t[k];
          const V3<T> r0 = load_v(a, strip_code(a, t, side, b));
          const V3<T> r1 = load_v(a, strip_code(a, t, side, b + 1));
          r = {r0.x + tt * (r1.x - r0.x), r0.y + tt * (r1.y - r0.y), r0.z + tt * (r1.z - r0.z)};
        } else {
          r = load_v(a, strip_code(a, t, side, pos));
        }
      }
      const int w = (wy + 1) * WS + wx + 1;
      win[0][w] = r.x;
      win[1][w] = r.y;
      win[2][w] = r.z;
    }
  }
  __syncthreads();

  // ---- compute ----------------------------------------------------------------------
  double s_mass = 0, s_en = 0, s_pens = 0, s_circ = 0, s_acirc = 0, s_cour = 0;
  if (own) {
    const int wc = (ly + 1) * WS + lx + 1;
    T ew[3], ee[3], es[3], en[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const T c = win[k][wc];
      ew[k] = T(0.5) * (win[k][wc - 1] + c);
      ee[k] = T(0.5) * (c + win[k][wc + 1]);
      es[k] = T(0.5) * (win[k][wc - WS] + c);
      en[k] = T(0.5) * (c + win[k][wc + WS]);
    }
    const size_t n1 = n + 1;
    const size_t cell = ((size_t)t * n + y) * n + x;
    // x-edge tables [T][3][n][n+1], y-edge tables [T][3][n+1][n]
    const size_t kx = (size_t)t * 3 * n * n1 + (size_t)y * n1 + x, sx = (size_t)n * n1;
    const size_t ky = (size_t)t * 3 * n1 * n + (size_t)y * n + x, sy = n1 * n;
    const T cW = (ew[0] * a.cdx[kx] + ew[1] * a.cdx[kx + sx]) + ew[2] * a.cdx[kx + 2 * sx];
    const T cE = (ee[0] * a.cdx[kx + 1] + ee[1] * a.cdx[kx + 1 + sx]) + ee[2] * a.cdx[kx + 1 + 2 * sx];
    const T cS = (es[0] * a.cdy[ky] + es[1] * a.cdy[ky + sy]) + es[2] * a.cdy[ky + 2 * sy];
    const T cN = (en[0] * a.cdy[ky + n] + en[1] * a.cdy[ky + n + sy]) + en[2] * a.cdy[ky + n + 2 * sy];
    const T invA = a.invA[cell];
    const T zeta = (((cS + cE) - cN) - cW) * invA;
    // normals [T][3][n+1]; lengths ex [T][n][n+1], ey [T][n+1][n]
    const T* mx = a.mx + (size_t)t * 3 * n1 + x;
    const T* my = a.my + (size_t)t * 3 * n1 + y;
    const size_t lxk = ((size_t)t * n + y) * n1 + x, lyk = ((size_t)t * n1 + y) * n + x;
    const T fW = ((ew[0] * mx[0] + ew[1] * mx[n1]) + ew[2] * mx[2 * n1]) * a.ex[lxk];
    const T fE = ((ee[0] * mx[1] + ee[1] * mx[n1 + 1]) + ee[2] * mx[2 * n1 + 1]) * a.ex[lxk + 1];
    const T fS = ((es[0] * my[0] + es[1] * my[n1]) + es[2] * my[2 * n1]) * a.ey[lyk];
    const T fN = ((en[0] * my[1] + en[1] * my[n1 + 1]) + en[2] * my[2 * n1 + 1]) * a.ey[lyk + n];
    const T delta = ((fE - fW) + (fN - fS)) * invA;
    const T pv = (zeta + a.omega2 * a.rz[cell]) / h;
    const size_t fs = (size_t)a.ntile * n * n;
    a.fields[cell] = zeta;
    a.fields[fs + cell] = delta;
    a.fields[2 * fs + cell] = pv;
    // invariant terms, fp64
    const double A = (double)a.area[cell], hd = (double)h;
    const double M0 = (double)m0, M1 = (double)m1, M2 = (double)m2;
    const double ke = 0.5 * ((M0 * M0 + M1 * M1) + M2 * M2) / hd;
    const double pe = 0.5 * (double)a.g * hd * hd + (double)a.g * hd * (double)a.b[cell];
    s_mass = hd * A;
    s_en = (ke + pe) * A;
    s_pens = 0.5 * (double)pv * (double)pv * hd * A;
    s_circ = (double)zeta * A;
    s_acirc = fabs((double)zeta) * A;
    const T v2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    s_cour = (double)((sqrt(v2) + sqrt(a.g * h)) * a.idxy[cell]);
  }
  // ---- block record: shuffle tree per wave, waves in order ----------------------
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s_mass += __shfl_down(s_mass, off);
    s_en += __shfl_down(s_en, off);
    s_pens += __shfl_down(s_pens, off);
    s_circ += __shfl_down(s_circ, off);
    s_acirc += __shfl_down(s_acirc, off);
    s_cour = nanmax(s_cour, __shfl_down(s_cour, off));
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    red[wave][0] = s_mass;
    red[wave][1] = s_en;
    red[wave][2] = s_pens;
    red[wave][3] = s_circ;
    red[wave][4] = s_acirc;
    red[wave][5] = s_cour;
    red[wave][6] = 0.0;
    red[wave][7] = 0.0;
  }
  __syncthreads();
  if (tid < NREC) {
    double r = red[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = tid == 5 ? nanmax(r, red[w][tid]) : r + red[w][tid];
    a.partials[(size_t)blockIdx.x * NREC + tid] = r;
  }
}

// records [nblocks][8] -> inv [8]: thread (chunk, k) folds component k of a
// contiguous chunk of blocks in block order, threads 0..7 then fold the chunks
// in order; component 5 is a maximum and is scaled by dt
__global__ __launch_bounds__(FOLD_CHUNKS * NREC) void derived_fold_kernel(const double* __restrict__ partials,
                                                                          int nblocks, double dt,
                                                                          double* __restrict__ inv) {
  __shared__ double part[FOLD_CHUNKS][NREC];
  const int k = threadIdx.x % NREC, c = threadIdx.x / NREC;
  const int per = (nblocks + FOLD_CHUNKS - 1) / FOLD_CHUNKS;
  const int b0 = min(c * per, nblocks), b1 = min(b0 + per, nblocks);
  double r = 0.0;
  for (int b = b0; b < b1; ++b) {
    const double p = partials[(size_t)b * NREC + k];
    r = k == 5 ? nanmax(r, p) : r + p;
  }
  part[c][k] = r;
  __syncthreads();
  if (threadIdx.x < NREC) {
    double s = part[0][k];
    for (int j = 1; j < FOLD_CHUNKS; ++j) s = k == 5 ? nanmax(s, part[j][k]) : s + part[j][k];
    inv[k] = k == 5 ? dt * s : s;
  }
}

template <typename T>
int launch(const DerivedDesc* d, hipStream_t s) {
  DArgs<T> a;
  a.Q = (const T*)d->Q;
  a.recv = (const T*)d->recv;
  a.gmap = d->gmap;
  a.cgmap = d->cgmap;
  a.pedge = d->pedge;
  a.pe_base = d->pe_base;
  a.pe_t = (const T*)d->pe_t;
  a.cdx = (const T*)d->cdx;
  a.cdy = (const T*)d->cdy;
  a.mx = (const T*)d->mx;
  a.my = (const T*)d->my;
  a.ex = (const T*)d->ex;
  a.ey = (const T*)d->ey;
  a.invA = (const T*)d->invA;
  a.area = (const T*)d->area;
  a.idxy = (const T*)d->idxy;
  a.b = (const T*)d->b;
  a.rz = (const T*)d->rz;
  a.fields = (T*)d->fields;
  a.partials = d->partials;
  a.ntile = d->ntile;
  a.n = d->n;
  a.S = d->S;
  a.mg = d->mg;
  a.pw = d->pw;
  a.nbx = a.nby = (d->n + DB - 1) / DB;
  a.g = (T)d->g;
  a.omega2 = (T)d->omega2;
  hipLaunchKernelGGL(derived_kernel<T>, dim3(d->nblocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(derived_fold_kernel, dim3(1), dim3(FOLD_CHUNKS * NREC), 0, s, (const double*)d->partials,
                     d->nblocks, d->dt, d->inv);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // namespace

extern "C" int stsp_derived_desc_size(void) { return (int)sizeof(DerivedDesc); }

extern "C" int stsp_derived_launch(int dtype, const DerivedDesc* d, hipStream_t stream) {
  if (!d || d->ntile <= 0 || d->n <= 0 || d->mg < 1) return 1;
  if (d->pw != d->n + 2 * d->mg || (long long)d->S != (long long)d->ntile * d->pw * d->pw) return 1;
  const int nb = (d->n + DB - 1) / DB;
  if ((long long)d->nblocks != (long long)d->ntile * nb * nb) return 1;
  if (!d->Q || !d->gmap || !d->cgmap || !d->pedge || !d->pe_base || !d->pe_t || !d->cdx || !d->cdy || !d->mx ||
      !d->my || !d->ex || !d->ey || !d->invA || !d->area || !d->idxy || !d->b || !d->rz || !d->fields ||
      !d->partials || !d->inv)
    return 1;
  if (d->nrecv < 0 || (d->nrecv > 0 && !d->recv)) return 1;
  if (dtype == 1) return launch<double>(d, stream);
  if (dtype == 0) return launch<float>(d, stream);
  return 2;
}
