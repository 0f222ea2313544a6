// Host check of the tagged-granule record codecs (ops/csrc/xg_codec.h), built
// and run by tests/test_xg_codec.py as plain C++: pack / unpack round-trip the
// exact bit patterns, every granule carries the tag, and the packed fp64
// form's 12-bit tag rejects the older records a slot can still hold.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "xg_codec.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                      \
  } while (0)

// splitmix64, fixed seed
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T> using Bits = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;
template <typename T> T from_bits(uint64_t b) {
  const Bits<T> v = (Bits<T>)b;
  T x;
  std::memcpy(&x, &v, sizeof(T));
  return x;
}
template <typename T> uint64_t to_bits(T x) {
  Bits<T> v;
  std::memcpy(&v, &x, sizeof(T));
  return v;
}

// all-zeros (+0), -0, all-ones (a NaN with full payload), quiet / signalling
// NaNs with payloads, infinities, smallest / largest denormals, 1.0
template <typename T> int special_bits(uint64_t (&out)[16]) {
  const int E = sizeof(T) == 8 ? 11 : 8, M = sizeof(T) == 8 ? 52 : 23;
  const uint64_t sign = 1ull << (E + M), expo = ((1ull << E) - 1) << M, mant = (1ull << M) - 1;
  int n = 0;
  out[n++] = 0;
  out[n++] = sign;
  out[n++] = sign | expo | mant;
  out[n++] = expo | mant;
  out[n++] = expo | (1ull << (M - 1)) | 0x2A5;
  out[n++] = expo | 1;
  out[n++] = sign | expo | (mant >> 1);
  out[n++] = expo;
  out[n++] = sign | expo;
  out[n++] = 1;
  out[n++] = sign | 1;
  out[n++] = mant;
  out[n++] = sign | mant;
  out[n++] = ((1ull << (E - 1)) - 1) << M;
  out[n++] = 0x5555555555555555ull & (sign | expo | mant);
  out[n++] = 0xAAAAAAAAAAAAAAAAull & (sign | expo | mant);
  return n;
}

// TAGBITS: width of the codec's tag field
template <class C, typename T, int F, int TAGBITS>
void roundtrip(const uint64_t (&bits)[F], unsigned tag, const char* name) {
  T q[F], r[F];
  for (int f = 0; f < F; ++f) q[f] = from_bits<T>(bits[f]);
  unsigned long long g[C::W];
  C::pack(q, tag, g);
  const unsigned mask = (unsigned)((1ull << TAGBITS) - 1);
  for (int k = 0; k < C::W; ++k) {
    CHECK(C::tag_ok(g[k], tag), "%s: granule %d of tag %u fails tag_ok", name, k, tag);
    CHECK(C::tag_of(g[k]) == (tag & mask), "%s: granule %d tag_of %u != %u", name, k, C::tag_of(g[k]), tag & mask);
    // the older records a two-slot buffer or a four-slot ring can still hold,
    // and the neighbours of the tag
    for (unsigned d : {1u, 2u, 3u, 4u})
      CHECK(!C::tag_ok(g[k], tag + d) && !C::tag_ok(g[k], tag - d), "%s: tag %u passes as %u +- %u", name, tag, tag, d);
  }
  C::unpack(g, r);
  for (int f = 0; f < F; ++f)
    CHECK(to_bits(r[f]) == to_bits(q[f]), "%s: field %d %016llx -> %016llx (tag %u)", name, f,
          (unsigned long long)to_bits(q[f]), (unsigned long long)to_bits(r[f]), tag);
}

template <class C, typename T, int F, int TAGBITS>
void check_codec(const char* name) {
  static_assert(C::W * 64 >= F * (int)sizeof(T) * 8 + C::W * TAGBITS, "payload and tags fit the granules");
  const unsigned tags[] = {0u, 1u, 2u, 3u, 4u, 5u, 4094u, 4095u, 4096u, 4097u, 4098u, 65535u, 65536u,
                           0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFF000u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
  uint64_t sp[16];
  const int ns = special_bits<T>(sp);
  uint64_t b[F];
  // every special pattern in every field, the other fields holding another one
  for (unsigned tag : tags)
    for (int f = 0; f < F; ++f)
      for (int i = 0; i < ns; ++i)
        for (int j = 0; j < ns; ++j) {
          for (int k = 0; k < F; ++k) b[k] = sp[j];
          b[f] = sp[i];
          roundtrip<C, T, F, TAGBITS>(b, tag, name);
        }
  // random patterns in every field, random tags across the 32-bit range
  for (int it = 0; it < 200000; ++it) {
    for (int k = 0; k < F; ++k) b[k] = rnd();
    roundtrip<C, T, F, TAGBITS>(b, (unsigned)rnd(), name);
  }
}

// the plain fp64 form, word for word: low word in granule 2 f, high word in 2 f + 1
void check_plain_word_order() {
  const double q[4] = {from_bits<double>(0x0123456789ABCDEFull), from_bits<double>(0xFEDCBA9876543210ull),
                       from_bits<double>(0x00000000FFFFFFFFull), from_bits<double>(0xFFFFFFFF00000000ull)};
  unsigned long long g[8];
  XgPlain<double, 4>::pack(q, 0xCAFEF00Du, g);
  const unsigned long long want[8] = {0xCAFEF00D89ABCDEFull, 0xCAFEF00D01234567ull, 0xCAFEF00D76543210ull,
                                      0xCAFEF00DFEDCBA98ull, 0xCAFEF00DFFFFFFFFull, 0xCAFEF00D00000000ull,
                                      0xCAFEF00D00000000ull, 0xCAFEF00DFFFFFFFFull};
  for (int k = 0; k < 8; ++k) CHECK(g[k] == want[k], "plain fp64 granule %d: %016llx != %016llx", k, g[k], want[k]);
  const float qf[1] = {from_bits<float>(0x89ABCDEFu)};
  unsigned long long gf[1];
  XgPlain<float, 1>::pack(qf, 7u, gf);
  CHECK(gf[0] == 0x0000000789ABCDEFull, "plain fp32 granule: %016llx", gf[0]);
}

// packed fp64: tag_ok(g, want) is false for the records want - 2 and want - 4
// (mod 4096) that a slot can hold instead of the one waited for
void check_packed_window() {
  const double q[4] = {1.0, -2.5, 3.25e-300, from_bits<double>(~0ull)};
  for (unsigned want = 0; want < 3 * 4096u; ++want)
    for (unsigned old : {2u, 4u}) {
      unsigned long long g[5];
      HX<double>::pack(q, want - old, g);
      for (int k = 0; k < 5; ++k)
        CHECK(!HX<double>::tag_ok(g[k], want), "packed fp64: record %u - %u passes as %u", want, old, want);
    }
}

}  // namespace

int main() {
  static_assert(XgPlain<double, 4>::W == 8 && XgPlain<float, 4>::W == 4 && XgPlain<double, 1>::W == 2 &&
                XgPlain<float, 1>::W == 1 && HX<double>::W == 5 && HX<float>::W == 4, "granules per record");
  check_codec<XgPlain<double, 4>, double, 4, 32>("plain fp64 F=4");
  check_codec<XgPlain<float, 4>, float, 4, 32>("plain fp32 F=4");
  check_codec<XgPlain<double, 1>, double, 1, 32>("plain fp64 F=1");
  check_codec<XgPlain<float, 1>, float, 1, 32>("plain fp32 F=1");
  check_codec<HX<double>, double, 4, 12>("packed fp64");
  check_codec<HX<float>, float, 4, 32>("packed fp32");
  check_plain_word_order();
  check_packed_window();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("xg codecs ok\n");
  return 0;
}
