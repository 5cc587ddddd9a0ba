// Self-test of kernels/atomic_plan.h on the CPU (no HIP): over small G, S and T, that the inverse of the
// slot map inverts, that every slot gets exactly c contributors per step, that the verifier's walk over a
// slot's contributors gives what a scatter in lane order gives, and that the packed and fp32 bounds hold for
// the largest n. Built plain and with ASan/UBSan (native/build.py), run by tests/test_atomic_check_ref.py.
// Prints "OK ..." and exits 0, or says what failed.
#include <cstdio>
#include <vector>

#include "../kernels/atomic_plan.h"

using namespace amdkube;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static bool same(const AtomicExpect& a, const AtomicExpect& b, uint32_t n) {
  for (int op = 0; op < AOP_COUNT; ++op)
    if (atomic_want_bits(a, op, n) != atomic_want_bits(b, op, n)) return false;
  return true;
}

int main() {
  long cases = 0;
  for (uint32_t seed : {0x5eedu, 1u, 0xffffffffu})
    for (uint32_t G : {1u, 2u, 64u, 256u, 1024u})
      for (uint32_t c = 1; c <= G; c *= 2)
        for (uint32_t T : {1u, 2u, 4u}) {
          const AtomicShape sh = atomic_shape(G, c, T);
          CHECK(sh.S * c == G && (1u << sh.lgS) == sh.S && sh.n == c * T && sh.cl * sh.SL == 256u);
          const uint32_t round = seed & 3u, key = atomic_key(seed, round), fm = atomic_f32_mask(sh.n);
          std::vector<AtomicExpect> scattered(sh.S);
          for (AtomicExpect& e : scattered) e.init();
          for (uint32_t i = 0; i < T; ++i) {
            const AtomicMap m = atomic_map(seed, round, i);
            CHECK(m.mul % 2 == 1 && m.mul * m.inv == 1u);
            std::vector<uint32_t> hits(sh.S, 0), ranks(G, 0);
            for (uint32_t g = 0; g < G; ++g) {
              const uint32_t p = atomic_position(m, g, G), s = p & (sh.S - 1), j = p >> sh.lgS;
              CHECK(p < G && atomic_lane_of(m, p, G) == g && j < c);
              ++hits[s];
              ++ranks[j * sh.S + s];
              scattered[s].add(atomic_operands(atomic_value(key, g, i), j, fm));
            }
            for (uint32_t s = 0; s < sh.S; ++s) CHECK(hits[s] == c);
            for (uint32_t q = 0; q < G; ++q) CHECK(ranks[q] == 1);   // every (slot, rank) exactly once
          }
          if (T == ATOMIC_STEPS || G <= 64)
            for (uint32_t s = 0; s < sh.S; ++s) CHECK(same(scattered[s], atomic_expect_slot(seed, round, G, c, s, T), sh.n));
          // merge: two halves of a slot's reduction combine to the whole
          AtomicExpect a = scattered[0], b;
          b.init();
          a.merge(b);
          CHECK(same(a, scattered[0], sh.n));
          ++cases;
        }

  // ---- bounds at every n up to the largest (G = 2^18, c = G, T = 4: n = 2^20)
  for (uint32_t n = 1; n <= (1u << 20); n *= 2) {
    const uint32_t fm = atomic_f32_mask(n);
    CHECK(static_cast<unsigned long long>(n) * fm < (1ull << 24));         // fp32: every partial sum an exact integer
    CHECK(fm >= 15u && ((fm + 1) & fm) == 0);
    CHECK(static_cast<unsigned long long>(n) * 0xffffffffull < (1ull << 53));   // f64 alike
  }
  unsigned bf_max = 0, h_max = 0;
  for (uint32_t v = 0; v < (1u << 18); ++v)
    for (uint32_t j : {0u, 7u, 8u, 15u, 16u, 1000u}) {
      const AtomicOperands o = atomic_operands(v * 0x9e3779b9u, j, 0xffu);
      const unsigned bl = o.pk_bf16 & 0xffffu, bh = o.pk_bf16 >> 16, hl = o.pk_f16 & 0xffffu, hh = o.pk_f16 >> 16;
      CHECK((j < 8) == (bl != 0) && (j < 8) == (bh != 0) && (j < 16) == (hl != 0) && (j < 16) == (hh != 0));
      bf_max = bl > bf_max ? bl : bf_max;
      bf_max = bh > bf_max ? bh : bf_max;
      h_max = hl > h_max ? hl : h_max;
      h_max = hh > h_max ? hh : h_max;
    }
  CHECK(bf_max == ATOMIC_PK_BF16_MAX && h_max == ATOMIC_PK_F16_MAX);
  CHECK(ATOMIC_STEPS * ATOMIC_PK_BF16_RANKS * bf_max <= 256 && ATOMIC_STEPS * ATOMIC_PK_F16_RANKS * h_max <= 2048);
  // the integer -> bf16 / f16 bit patterns, against the formats' definitions
  for (uint32_t x = 0; x <= 2048; ++x) {
    const uint32_t h = atomic_f16_bits(x);
    const double back = x == 0 ? 0.0 : (1.0 + (h & 0x3ff) / 1024.0) * static_cast<double>(1ull << ((h >> 10) - 15));
    CHECK(h < 0x7c00u && back == x);
    if (x <= 256) {
      const uint32_t bits = atomic_bf16_bits(x) << 16;
      CHECK(__builtin_bit_cast(float, bits) == static_cast<float>(x));
    }
  }
  CHECK(atomic_inverse(1u) == 1u && atomic_inverse(0xffffffffu) == 0xffffffffu);

  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("OK %ld shapes\n", cases);
  return 0;
}
