// Record codecs of the tagged-granule hand-off (xg_ring.h): a record of field
// values <-> W 64-bit granules, each {tag, payload}.  Integer and bit_cast
// code only, so a plain host compiler can include this header
// (tests/xg_codec_check.cpp checks the packing bit for bit).
//
// Both codecs share one interface:
//   W                   granules per record
//   pack(q, tag, g)     the record q with `tag` in every granule
//   unpack(g, q)        the exact bit patterns pack() was given
//   tag_ok(g, want)     granule g carries tag `want`
//   tag_of(g)           the tag of g (failure reports)
#pragma once

#ifdef __HIPCC__
#define XG_HD __host__ __device__ __forceinline__
#else
#define XG_HD inline
#endif

// Plain form (stage and streaming-stage kernels): one 32-bit word of the record
// per granule under a 32-bit tag.  An 8-byte value travels low word first
// (granule 2 f, then 2 f + 1).
template <typename T, int F> struct XgPlain {
  static constexpr int G = sizeof(T) / 4;   // granules per value
  static constexpr int W = F * G;
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit values");
  XG_HD static void pack(const T (&q)[F], unsigned tag, unsigned long long (&g)[W]) {
    const unsigned long long t = (unsigned long long)tag << 32;
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if constexpr (G == 2) {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, q[f]);
        g[2 * f] = t | (b & 0xFFFFFFFFull);
        g[2 * f + 1] = t | (b >> 32);
      } else {
        g[f] = t | __builtin_bit_cast(unsigned, q[f]);
      }
    }
  }
  XG_HD static bool tag_ok(unsigned long long g, unsigned want) { return (unsigned)(g >> 32) == want; }
  XG_HD static unsigned tag_of(unsigned long long g) { return (unsigned)(g >> 32); }
  XG_HD static void unpack(const unsigned long long (&g)[W], T (&q)[F]) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if constexpr (G == 2)
        q[f] = __builtin_bit_cast(T, (g[2 * f + 1] << 32) | (g[2 * f] & 0xFFFFFFFFull));
      else
        q[f] = __builtin_bit_cast(T, (unsigned)g[f]);
    }
  }
};

// Packed form (fused step: its xGMI ring and its in-launch hand-off buffer):
// the 4 field values of a cell.  fp64: 5 granules of a 12-bit tag and 52
// payload bits (the 256 value bits in 5 x 52 = 260), against 8 granules in the
// plain form; fp32: the plain form.  12 tag bits suffice: a slot holds this
// step's record (tag want) or the one it replaces, two (two-slot hand-off
// buffer) or four (four-slot ring) steps older, i.e. want - 2 or want - 4 mod
// 4096, never anything else (profiles/r6_handoff).
template <typename T> struct HX;
template <> struct HX<double> {
  static constexpr int W = 5;
  static constexpr unsigned long long M52 = (1ull << 52) - 1;
  XG_HD static void pack(const double (&q)[4], unsigned tag, unsigned long long (&g)[5]) {
    const unsigned long long u0 = __builtin_bit_cast(unsigned long long, q[0]);
    const unsigned long long u1 = __builtin_bit_cast(unsigned long long, q[1]);
    const unsigned long long u2 = __builtin_bit_cast(unsigned long long, q[2]);
    const unsigned long long u3 = __builtin_bit_cast(unsigned long long, q[3]);
    const unsigned long long t = (unsigned long long)(tag & 0xFFFu) << 52;
    g[0] = t | (u0 & M52);
    g[1] = t | (u0 >> 52) | ((u1 << 12) & M52);
    g[2] = t | (u1 >> 40) | ((u2 << 24) & M52);
    g[3] = t | (u2 >> 28) | ((u3 << 36) & M52);
    g[4] = t | (u3 >> 16);
  }
  XG_HD static bool tag_ok(unsigned long long g, unsigned want) { return (unsigned)(g >> 52) == (want & 0xFFFu); }
  XG_HD static unsigned tag_of(unsigned long long g) { return (unsigned)(g >> 52); }
  XG_HD static void unpack(const unsigned long long (&g)[5], double (&q)[4]) {
    const unsigned long long c0 = g[0] & M52, c1 = g[1] & M52, c2 = g[2] & M52, c3 = g[3] & M52, c4 = g[4] & M52;
    q[0] = __builtin_bit_cast(double, c0 | (c1 << 52));
    q[1] = __builtin_bit_cast(double, (c1 >> 12) | (c2 << 40));
    q[2] = __builtin_bit_cast(double, (c2 >> 24) | (c3 << 28));
    q[3] = __builtin_bit_cast(double, (c3 >> 36) | (c4 << 16));
  }
};
template <> struct HX<float> : XgPlain<float, 4> {};
