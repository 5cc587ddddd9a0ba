// Host-side policy shared by the GPU integrity checks and the burn: how a run is calibrated to its
// duration, where the self-test flips go, how a comma list is split and a list of unit names becomes a
// mask, where a wave ran (CuLocation) and which CUs and SIMDs the launches of a run have covered
// (CuCoverage); and mix32, the hash that host and device share.
// Plain C++17 with no HIP include, so native/check_core_selftest.cpp checks it on the CPU, plain and
// under ASan/UBSan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

// for what the host and a kernel both compute: empty without HIP
#if defined(__HIP__)
#define AK_HOST_DEVICE __attribute__((host)) __attribute__((device))
#else
#define AK_HOST_DEVICE
#endif

namespace amdkube {

// The project's one integer hash: every pattern, seed and self-test position is made of it, on the device
// and in the host code that predicts what the device wrote.
AK_HOST_DEVICE inline __attribute__((always_inline)) uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the checks' hash of (seed, workgroup, index)
AK_HOST_DEVICE inline __attribute__((always_inline)) uint32_t mix32(uint32_t seed, uint32_t block, uint32_t index) {
  return mix32(mix32(seed ^ (0x9e3779b9u * (block + 1))) + index);
}

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

// "a, b, c", for the messages that list a check's units
inline std::string unit_names(const char* const* names, int n) {
  std::string all;
  for (int u = 0; u < n; ++u) all += std::string(u ? ", " : "") + names[u];
  return all;
}

// "lds,trans" -> mask, unit u of `names` being bit 1 << u; throws std::invalid_argument on an unknown or empty name
inline int unit_mask(const std::string& list, const char* const* names, int n) {
  int mask = 0;
  for (const std::string& name : split_list(list)) {
    int u = 0;
    while (u < n && name != names[u]) ++u;
    if (u == n) throw std::invalid_argument("unknown unit '" + name + "': expected a comma list over " + unit_names(names, n));
    mask |= 1 << u;
  }
  return mask;
}

// Where a wave runs, decoded from its raw HW_ID and XCC_ID words (the field layout and what an MI355X shows
// in them: cu_check.h). For the checks that say where an error was seen.
struct CuLocation {
  int xcc = 0, se = 0, sh = 0, cu = 0;
  uint32_t key() const { return static_cast<uint32_t>(xcc) << 12 | se << 8 | sh << 4 | cu; }
  static CuLocation of_key(uint32_t key) {
    CuLocation l;
    l.xcc = key >> 12;
    l.se = (key >> 8) & 15;
    l.sh = (key >> 4) & 15;
    l.cu = key & 15;
    return l;
  }
};

inline CuLocation cu_decode_location(uint32_t hw_id, uint32_t xcc_id) {
  CuLocation l;
  l.xcc = xcc_id & 15u;
  l.cu = (hw_id >> 8) & 15u;
  l.sh = (hw_id >> 12) & 1u;
  l.se = (hw_id >> 13) & 7u;
  return l;
}

inline int cu_decode_simd(uint32_t hw_id) { return static_cast<int>((hw_id >> 4) & 3u); }

struct CuBadCu {
  CuLocation where;
  unsigned long long errors = 0;
};

// The places the launches of a per-CU check have run on, and the errors counted on each. A workgroup owns
// its CU and reports `waves` raw HW_ID words (one per reporting wave, the first of wave 0) and then the XCC_ID.
struct CuCoverage {
  int waves;
  std::set<uint32_t> seen, seen_simds;             // location keys; key << 2 | SIMD
  std::map<uint32_t, unsigned long long> bad;      // location key -> errors
  explicit CuCoverage(int waves_) : waves(waves_) {}
  // one finished launch: loc is [blocks][waves + 1], block_errors [blocks]. Says whether any workgroup
  // counted errors, that is whether the device's counts have to be cleared before the next launch.
  bool add(const std::vector<uint32_t>& loc, const std::vector<unsigned>& block_errors) {
    bool any = false;
    for (size_t b = 0; b < block_errors.size(); ++b) {
      const uint32_t* w = &loc[b * (waves + 1)];
      const uint32_t key = cu_decode_location(w[0], w[waves]).key();
      seen.insert(key);
      for (int v = 0; v < waves; ++v) seen_simds.insert(cu_decode_location(w[v], w[waves]).key() << 2 | cu_decode_simd(w[v]));
      if (block_errors[b]) {
        bad[key] += block_errors[b];
        any = true;
      }
    }
    return any;
  }
  int cus_covered() const { return static_cast<int>(seen.size()); }
  int simds_covered() const { return static_cast<int>(seen_simds.size()); }
  int xccs() const {
    std::set<uint32_t> x;
    for (uint32_t key : seen) x.insert(key >> 12);
    return static_cast<int>(x.size());
  }
  // the distinct places, sorted
  std::vector<CuLocation> locations() const {
    std::vector<CuLocation> l;
    for (uint32_t key : seen) l.push_back(CuLocation::of_key(key));
    return l;
  }
  // the first `cap` CUs with errors, in key order
  std::vector<CuBadCu> bad_cus(size_t cap = 16) const {
    std::vector<CuBadCu> out;
    for (const auto& kv : bad) {
      if (out.size() == cap) break;
      out.push_back(CuBadCu{CuLocation::of_key(kv.first), kv.second});
    }
    return out;
  }
};

}  // namespace amdkube
