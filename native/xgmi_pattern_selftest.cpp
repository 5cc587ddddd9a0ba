// Self-test of kernels/xgmi_pattern.h on the CPU (no HIP): for every rank count from 1 to 64 the fp32 sum of
// the ranks' values, taken in ascending, descending and pairwise order, is the expected value bit for bit,
// at element indices on both sides of 2^32; the term stays below 4096 and depends on both halves of the
// index. Built plain and with ASan/UBSan (native/build.py), run by tests/test_xgmi_verify_ref.py, which
// holds the table printed below against the numpy mirror (amdkube/ops/xgmiverify.py). Prints "OK ..." last
// and exits 0, or says what failed.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../kernels/xgmi_pattern.h"

using namespace amdkube;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

// the sum of v[lo, hi) as a tree: what a recursive-halving reduction computes
static float pairwise(const std::vector<float>& v, size_t lo, size_t hi) {
  if (hi - lo == 1) return v[lo];
  const size_t mid = lo + (hi - lo) / 2;
  const volatile float a = pairwise(v, lo, mid), b = pairwise(v, mid, hi);
  return a + b;
}

static std::vector<uint64_t> spread_of_indices() {
  std::vector<uint64_t> es;
  for (uint64_t e = 0; e < 300; ++e) es.push_back(e);
  for (uint64_t base : {uint64_t(1) << 24, uint64_t(1) << 31, uint64_t(1) << 32, uint64_t(5) << 32, uint64_t(1) << 40,
                        ~uint64_t(0) - 16})
    for (uint64_t d = 0; d < 16; ++d) es.push_back(base - 3 + d);
  for (uint64_t i = 0; i < 2000; ++i) es.push_back(i * 0x9e3779b97f4a7c15ull);   // all over the 64 bits
  return es;
}

int main() {
  CHECK(mix32(0) == 0 && mix32(1) == 0x688990c0u);
  CHECK(XGMI_MAX_RANKS == 64);
  const std::vector<uint64_t> es = spread_of_indices();
  for (uint32_t seed : {0x5eedu, 12345u, 0u, 0xffffffffu}) {
    std::set<uint32_t> terms;
    for (uint64_t e : es) {
      const uint32_t t = xgmi_term(seed, e);
      CHECK(t < 4096);
      terms.insert(t);
      for (int n = 1; n <= XGMI_MAX_RANKS; ++n) {
        std::vector<float> v(n);
        for (int r = 0; r < n; ++r) v[r] = xgmi_value(seed, r, e);
        volatile float up = 0, down = 0;   // volatile: every partial sum is rounded to fp32, as a device's is
        for (int r = 0; r < n; ++r) up = up + v[r];
        for (int r = n - 1; r >= 0; --r) down = down + v[r];
        const uint32_t want = bits(xgmi_want(seed, n, e));
        if (bits(up) != want || bits(down) != want || bits(pairwise(v, 0, n)) != want) {
          std::fprintf(stderr, "FAILED: seed %u n %d e %llu\n", seed, n, static_cast<unsigned long long>(e));
          ++failures;
        }
      }
      CHECK(bits(xgmi_value(seed, 0, e)) == bits(1.0f + 0.5f * t) && xgmi_want(seed, 1, e) == xgmi_value(seed, 0, e));
    }
    CHECK(terms.size() > 1500);   // ~2400 indices drawn from 4096 values: not a handful of them
    // both halves of the index count
    CHECK(xgmi_term(seed, 7) != xgmi_term(seed, (uint64_t(1) << 32) + 7) || xgmi_term(seed, 8) != xgmi_term(seed, (uint64_t(1) << 32) + 8));
  }
  CHECK(xgmi_want(0x5eedu, 64, 0) <= 133120.0f && xgmi_value(0x5eedu, 63, 0) <= 64.0f + 0.5f * 4095);
  // the table tests/test_xgmi_verify_ref.py compares with the numpy mirror
  for (uint32_t seed : {0x5eedu, 12345u, 0u, 0xffffffffu})
    for (uint64_t e : {uint64_t(0), uint64_t(1), uint64_t(7), uint64_t(4096), uint64_t(262143), (uint64_t(1) << 32) - 1,
                       uint64_t(1) << 32, (uint64_t(3) << 32) + 5, ~uint64_t(0)}) {
      for (int rank : {0, 1, 63})
        std::printf("value %u %d %llu %u\n", seed, rank, static_cast<unsigned long long>(e), bits(xgmi_value(seed, rank, e)));
      for (int n : {1, 2, 3, 8, 64})
        std::printf("want %u %d %llu %u\n", seed, n, static_cast<unsigned long long>(e), bits(xgmi_want(seed, n, e)));
    }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK xgmi_pattern: term, value, want; sums of 1..64 ranks in three orders\n");
  return 0;
}
