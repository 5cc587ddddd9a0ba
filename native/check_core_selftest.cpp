// Self-test of kernels/check_core.h on the CPU (no HIP): the calibration against the launch sequences
// of the loops it replaced, the flip positions against a second, naive transcription of the arithmetic
// the two checks used to carry, and the list splitter. Built plain and with ASan/UBSan
// (native/build.py), run by tests/test_check_core.py. Prints "OK ..." and exits 0, or says what failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "../kernels/check_core.h"

using namespace amdkube;
using Calls = std::vector<std::pair<int, int>>;
using ull = unsigned long long;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

// a launch that lasts rounds * c ms and records how it was called
struct Fake {
  double c;
  Calls calls;
  double operator()(int rounds, int flips) {
    calls.push_back({rounds, flips});
    return rounds * c;
  }
};

// ---- the loops as the drivers of the two checks and the burn had them, word for word
static Calibrated old_check_loop(Fake& timed, int first, int rounds, double target_ms, int flips) {
  double ms;
  if (rounds > 0) {
    ms = timed(rounds, flips);
  } else {
    rounds = first;
    ms = timed(rounds, 0);
    while (ms < 20.0 && rounds < (1 << 26)) {
      rounds *= 4;
      ms = timed(rounds, 0);
    }
    const bool longer = target_ms > ms && ms > 0;
    if (longer) {
      const double want = rounds * (target_ms / ms);
      rounds = want > 2.0e9 ? 2000000000 : static_cast<int>(want);
    }
    if (longer || flips > 0) ms = timed(rounds, flips);
  }
  return {rounds, ms};
}

static Calibrated old_burn_loop(Fake& run, double target_ms) {
  int iters = 2000;
  double ms = run(iters, 0);
  while (ms < 20.0 && iters < 200000000) {
    iters *= 4;
    ms = run(iters, 0);
  }
  if (target_ms > ms && ms > 0) {
    double scale = target_ms / ms;
    double want = iters * scale;
    iters = want > 2.0e9 ? 2000000000 : static_cast<int>(want);
    ms = run(iters, 0);
  }
  return {iters, ms};
}

static void same_as_check_loop(double c, int first, int rounds, double target_ms, int flips) {
  Fake a{c, {}}, b{c, {}};
  const Calibrated got = calibrate(a, first, 1 << 26, rounds, target_ms, flips), want = old_check_loop(b, first, rounds, target_ms, flips);
  CHECK(a.calls == b.calls && got.rounds == want.rounds && got.ms == want.ms);
}

static void test_calibrate() {
  {  // calibrated and scaled, the flips in the last launch only
    Fake f{0.01, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 0, 200.0, 5);
    CHECK((f.calls == Calls{{256, 0}, {1024, 0}, {4096, 0}, {20000, 5}}));
    CHECK(r.rounds == 20000 && r.ms == 20000 * 0.01);
  }
  {  // the calibration launch already reaches the target: it is the result
    Fake f{0.01, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 0, 30.0, 0);
    CHECK((f.calls == Calls{{256, 0}, {1024, 0}, {4096, 0}}));
    CHECK(r.rounds == 4096 && r.ms == 4096 * 0.01);
  }
  {  // ... unless there are flips to run
    Fake f{0.01, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 0, 30.0, 5);
    CHECK((f.calls == Calls{{256, 0}, {1024, 0}, {4096, 0}, {4096, 5}}));
    CHECK(r.rounds == 4096 && r.ms == 4096 * 0.01);
  }
  {  // a given round count is one launch
    Fake f{0.01, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 7, 200.0, 3);
    CHECK((f.calls == Calls{{7, 3}}));
    CHECK(r.rounds == 7 && r.ms == 7 * 0.01);
  }
  {  // a launch that takes no time: stops at the cap and does not scale
    Fake f{0.0, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 0, 200.0, 0);
    CHECK(f.calls.size() == 10 && f.calls.back() == std::make_pair(1 << 26, 0) && f.calls[8].first < (1 << 26));
    CHECK(r.rounds == (1 << 26) && r.ms == 0);
    Fake g{0.0, {}};
    calibrate(g, 16, 1 << 26, 0, 200.0, 0);
    CHECK(g.calls.size() == 12 && g.calls.back() == std::make_pair(1 << 26, 0));
  }
  {  // a target beyond 2e9 rounds clamps
    Fake f{0.01, {}};
    const Calibrated r = calibrate(f, 256, 1 << 26, 0, 1.0e9, 0);
    CHECK(f.calls.back() == std::make_pair(2000000000, 0) && r.rounds == 2000000000);
  }
  {  // the per-CU check's first count, long already: no x4 step
    Fake f{2.0, {}};
    const Calibrated r = calibrate(f, 16, 1 << 26, 0, 200.0, 0);
    CHECK((f.calls == Calls{{16, 0}, {100, 0}}) && r.rounds == 100 && r.ms == 200.0);
  }
  // the same sequences as the loop of the checks over a grid of rates, targets and flips
  for (double c : {0.0, 1e-7, 0.0007, 0.01, 0.3, 2.0, 25.0})
    for (int first : {256, 16})
      for (double target : {0.0, 19.0, 30.0, 200.0, 1.0e9})
        for (int flips : {0, 5}) {
          same_as_check_loop(c, first, 0, target, flips);
          same_as_check_loop(c, first, 7, target, flips);
        }
  // the burn: 2000 first, 200000000 the cap, no flips
  for (double c : {0.0, 1e-9, 1e-6, 0.0004, 0.01, 1.0})
    for (double target : {0.0, 100.0, 200.0, 1.0e9}) {
      Fake a{c, {}}, b{c, {}};
      const Calibrated got = calibrate(a, 2000, 200000000, 0, target, 0), want = old_burn_loop(b, target);
      CHECK(a.calls == b.calls && got.rounds == want.rounds && got.ms == want.ms);
    }
  {
    Fake f{1.0 / 2048, {}};  // 128000 iterations last 62.5 ms, a quarter of the target
    const Calibrated r = calibrate(f, 2000, 200000000, 0, 250.0, 0);
    CHECK((f.calls == Calls{{2000, 0}, {8000, 0}, {32000, 0}, {128000, 0}, {512000, 0}}) && r.rounds == 512000 && r.ms == 250.0);
    Fake z{0.0, {}};
    calibrate(z, 2000, 200000000, 0, 200.0, 0);
    CHECK(z.calls.back().first == 2000 * 262144 && z.calls.back().first >= 200000000 && z.calls[z.calls.size() - 2].first < 200000000);
  }
}

// ---- the flip positions as the constructors of the two runs had them
static ull old_gcd(ull a, ull b) {
  while (b) {
    const ull r = a % b;
    a = b;
    b = r;
  }
  return a;
}

static std::vector<uint32_t> old_mfma_positions(uint32_t seed, int blocks) {
  const ull positions = static_cast<ull>(blocks) * (64 * 64);
  const ull base = (seed * 2654435761ull + 0x5bd1e995u) % positions;
  ull stride = (((seed ^ 0x9e3779b9u) * 0x85ebca6bull) % positions) | 1;
  while (old_gcd(stride, positions) != 1) stride += 2;
  std::vector<uint32_t> pos(4096);
  for (size_t i = 0; i < pos.size(); ++i) pos[i] = static_cast<uint32_t>((base + i * stride) % positions);
  return pos;
}

static std::vector<uint32_t> old_cu_positions(uint32_t seed, int blocks, int units) {
  const ull small = static_cast<ull>(blocks) * 1024;
  const ull large = static_cast<ull>(blocks) * 40960;
  const ull base = seed * 2654435761ull + 0x5bd1e995u;
  ull stride = (((seed ^ 0x9e3779b9u) * 0x85ebca6bull) % small) | 1;
  while (old_gcd(stride, large) != 1) stride += 2;
  int slot_unit[3], n_en = 0;
  for (int u = 0; u < 3; ++u)
    if (units & (1 << u)) slot_unit[n_en++] = u;
  std::vector<uint32_t> pos(4096);
  for (size_t i = 0; i < pos.size(); ++i)
    pos[i] = static_cast<uint32_t>((base + i * stride) % (slot_unit[i % n_en] == 0 ? large : small));
  return pos;
}

// the positions of every n-th flip from `first` on are distinct and below `modulus`
static bool distinct_below(const std::vector<uint32_t>& pos, size_t first, size_t n, ull modulus) {
  std::set<uint32_t> seen;
  for (size_t i = first; i < pos.size(); i += n) {
    if (pos[i] >= modulus || !seen.insert(pos[i]).second) return false;
  }
  return true;
}

static void test_flip_positions() {
  for (uint32_t seed : {0x5eedu, 0u, 1u, 0xffffffffu})
    for (int blocks : {1024, 4}) {  // the MI355X, and a device of one CU
      const ull tiles = static_cast<ull>(blocks) * 4096;
      const std::vector<uint32_t> want = old_mfma_positions(seed, blocks);
      CHECK(distinct_below(want, 0, 1, tiles));  // the reference itself, 4096 of 16384 positions at 4 blocks
      const std::vector<uint32_t> got = flip_positions(seed, 4096, tiles);
      CHECK(got == want);
      CHECK(distinct_below(got, 0, 1, tiles));
      const ull small = static_cast<ull>(blocks) * 1024, large = static_cast<ull>(blocks) * 40960;
      for (int units = 1; units <= 7; ++units) {
        std::vector<ull> slot_mod;
        for (int u = 0; u < 3; ++u)
          if (units & (1 << u)) slot_mod.push_back(u == 0 ? large : small);
        const std::vector<uint32_t> cu_want = old_cu_positions(seed, blocks, units);
        const std::vector<uint32_t> cu_got = flip_positions(seed, 4096, small, large, slot_mod);
        CHECK(cu_got == cu_want);
        for (size_t s = 0; s < slot_mod.size(); ++s) {
          CHECK(distinct_below(cu_want, s, slot_mod.size(), slot_mod[s]));
          CHECK(distinct_below(cu_got, s, slot_mod.size(), slot_mod[s]));
        }
      }
    }
}

static void test_split_list() {
  using L = std::vector<std::string>;
  CHECK((split_list("a") == L{"a"}));
  CHECK((split_list("a,b") == L{"a", "b"}));
  CHECK((split_list("") == L{""}));
  CHECK((split_list("a,") == L{"a", ""}));
  CHECK((split_list(",a") == L{"", "a"}));
  CHECK((split_list("lds,valu,trans") == L{"lds", "valu", "trans"}));
}

int main() {
  test_calibrate();
  test_flip_positions();
  test_split_list();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK check_core: calibrate, flip_positions, split_list\n");
  return 0;
}
