// Host-side policy shared by the GPU integrity checks (mfma_check.h, cu_check.h) and the burn: how a
// run is calibrated to its duration, where the self-test flips go, how a comma list is split.
// Plain C++17 with no HIP include, so native/check_core_selftest.cpp checks it on the CPU, plain and
// under ASan/UBSan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace amdkube {

struct Calibrated {
  int rounds;
  double ms;  // of the last launch
};

// timed(rounds, flips) -> ms is one timed launch. rounds > 0: one launch of exactly that many rounds.
// rounds <= 0: a warm-up launch of `first_rounds` (code-object load and clock ramp inflate it), then
// four times as many until a launch is long enough (>= 20 ms) that launch overhead does not skew the
// rate, or `cap` is reached; the count is then scaled to ~target_ms. The self-test flips go into the
// last launch only.
template <class Timed>
inline Calibrated calibrate(Timed&& timed, int first_rounds, int cap, int rounds, double target_ms, int flips) {
  if (rounds > 0) return {rounds, timed(rounds, flips)};
  rounds = first_rounds;
  double ms = timed(rounds, 0);
  while (ms < 20.0 && rounds < cap) {
    rounds *= 4;
    ms = timed(rounds, 0);
  }
  const bool longer = target_ms > ms && ms > 0;
  if (longer) {
    const double want = rounds * (target_ms / ms);
    rounds = want > 2.0e9 ? 2000000000 : static_cast<int>(want);
  }
  if (longer || flips > 0) ms = timed(rounds, flips);
  return {rounds, ms};
}

// Self-test flip positions: flip i sits at (base + i * stride) mod slot_mod[i % slot_mod.size()], base
// and stride hashed from the seed. The stride is odd, drawn below `small` and bumped until coprime to
// `large`; every modulus divides `large`, so the positions that share a modulus are distinct while
// there are no more of them than the modulus. The base is below 1.15e19 and i * stride many orders
// below the 7e18 left under 2^64, so the sum does not wrap and reducing the base first changes nothing.
inline std::vector<uint32_t> flip_positions(uint32_t seed, size_t count, unsigned long long small, unsigned long long large,
                                            const std::vector<unsigned long long>& slot_mod) {
  auto gcd = [](unsigned long long a, unsigned long long b) {
    while (b) {
      const unsigned long long r = a % b;
      a = b;
      b = r;
    }
    return a;
  };
  const unsigned long long base = seed * 2654435761ull + 0x5bd1e995u;
  unsigned long long stride = (((seed ^ 0x9e3779b9u) * 0x85ebca6bull) % small) | 1;
  while (gcd(stride, large) != 1) stride += 2;
  std::vector<uint32_t> pos(count);
  for (size_t i = 0; i < count; ++i) pos[i] = static_cast<uint32_t>((base + i * stride) % slot_mod[i % slot_mod.size()]);
  return pos;
}

// one modulus for every flip
inline std::vector<uint32_t> flip_positions(uint32_t seed, size_t count, unsigned long long modulus) {
  return flip_positions(seed, count, modulus, modulus, {modulus});
}

// "a,b" -> {"a", "b"}. Empty names are kept ("" -> {""}, "a," -> {"a", ""}): the caller rejects them.
inline std::vector<std::string> split_list(const std::string& list) {
  std::vector<std::string> names;
  for (size_t at = 0; at <= list.size();) {
    size_t end = list.find(',', at);
    if (end == std::string::npos) end = list.size();
    names.push_back(list.substr(at, end - at));
    at = end + 1;
  }
  return names;
}

}  // namespace amdkube
