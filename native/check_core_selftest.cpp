// Self-test of kernels/check_core.h on the CPU (no HIP): the calibration against the launch sequences
// of the loops it replaced, the flip positions against a second, naive transcription of the arithmetic
// the two checks used to carry, the list splitter and the unit lists, the places and their keys, the
// coverage bookkeeping of the per-CU checks against a naive loop, and the check programs' command line
// (kernels/check_cli.h) on argv arrays. Built plain and with ASan/UBSan (native/build.py), run by
// tests/test_check_core.py. Prints "OK ..." and exits 0, or says what failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../kernels/check_cli.h"

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

// ---- unit lists
static void test_unit_mask() {
  const char* const names[4] = {"a", "bb", "c", "dd"};
  for (int mask = 1; mask < 16; ++mask) {  // every subset, ascending and descending; a repeated name changes nothing
    std::string up, down;
    for (int u = 0; u < 4; ++u)
      if (mask & (1 << u)) {
        up += (up.empty() ? "" : ",") + std::string(names[u]);
        down = names[u] + (down.empty() ? "" : "," + down);
      }
    CHECK(unit_mask(up, names, 4) == mask && unit_mask(down, names, 4) == mask && unit_mask(up + "," + down, names, 4) == mask);
  }
  CHECK(unit_names(names, 4) == "a, bb, c, dd" && unit_names(names, 1) == "a");
  auto refused = [&](const std::string& list, const std::string& name, int n) {
    try {
      unit_mask(list, names, n);
    } catch (const std::invalid_argument& e) {
      return std::string(e.what()) == "unknown unit '" + name + "': expected a comma list over " + unit_names(names, n);
    }
    return false;
  };
  CHECK(refused("x", "x", 4) && refused("a,x,c", "x", 4) && refused("", "", 4) && refused("a,", "", 4) && refused(",a", "", 4));
  CHECK(refused("A", "A", 4) && refused("a ", "a ", 4) && refused("dd", "dd", 3));  // exact names, of the first n only
  try {
    unit_mask("lds,foo", std::vector<const char*>{"lds", "valu", "trans"}.data(), 3);
    CHECK(false);
  } catch (const std::invalid_argument& e) {
    CHECK(std::string(e.what()) == "unknown unit 'foo': expected a comma list over lds, valu, trans");
  }
}

// ---- places
static void test_location() {
  for (int xcc = 0; xcc < 16; ++xcc)
    for (int se = 0; se < 8; ++se)
      for (int sh = 0; sh < 2; ++sh)
        for (int cu = 0; cu < 16; ++cu) {
          const uint32_t hw = static_cast<uint32_t>(se) << 13 | sh << 12 | cu << 8;
          const uint32_t noise = 0xffff00ffu;  // wave, SIMD, pipe, thread group, VM, queue, state, ME: no part of a place
          const CuLocation l = cu_decode_location(hw | noise, static_cast<uint32_t>(xcc) | 0xfffffff0u);
          CHECK(l.xcc == xcc && l.se == se && l.sh == sh && l.cu == cu);
          CHECK(l.key() == (static_cast<uint32_t>(xcc) << 12 | se << 8 | sh << 4 | cu));
          const CuLocation back = CuLocation::of_key(l.key());
          CHECK(back.xcc == xcc && back.se == se && back.sh == sh && back.cu == cu && back.key() == l.key());
        }
  for (uint32_t simd = 0; simd < 4; ++simd) CHECK(cu_decode_simd(0xffffffcfu | simd << 4) == static_cast<int>(simd));
}

static uint32_t hw_word(int se, int cu, int simd, int wave = 0) { return static_cast<uint32_t>(se) << 13 | cu << 8 | simd << 4 | wave; }

// what CuCoverage keeps, by the plainest loops over everything the launches reported
struct NaiveCoverage {
  int waves;
  std::vector<std::vector<uint32_t>> locs;
  std::vector<std::vector<unsigned>> errs;
  bool agrees(const CuCoverage& c) const {
    std::vector<uint32_t> keys, simd_keys, xccs;
    std::vector<std::pair<uint32_t, ull>> bad;
    auto add = [](std::vector<uint32_t>& v, uint32_t x) {
      if (std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x);
    };
    for (size_t l = 0; l < locs.size(); ++l)
      for (size_t b = 0; b < errs[l].size(); ++b) {
        const uint32_t* w = &locs[l][b * (waves + 1)];
        const uint32_t xcc = w[waves] & 15u;
        auto key = [&](uint32_t hw) { return xcc << 12 | ((hw >> 13) & 7u) << 8 | ((hw >> 12) & 1u) << 4 | ((hw >> 8) & 15u); };
        add(keys, key(w[0]));
        add(xccs, xcc);
        for (int v = 0; v < waves; ++v) add(simd_keys, key(w[v]) << 2 | ((w[v] >> 4) & 3u));
        if (!errs[l][b]) continue;
        size_t at = 0;
        while (at < bad.size() && bad[at].first != key(w[0])) ++at;
        if (at == bad.size()) bad.push_back({key(w[0]), 0});
        bad[at].second += errs[l][b];
      }
    std::sort(keys.begin(), keys.end());
    std::sort(bad.begin(), bad.end());
    if (bad.size() > 16) bad.resize(16);
    const std::vector<CuLocation> places = c.locations();
    const std::vector<CuBadCu> bad_cus = c.bad_cus();
    bool ok = c.cus_covered() == static_cast<int>(keys.size()) && c.simds_covered() == static_cast<int>(simd_keys.size()) &&
              c.xccs() == static_cast<int>(xccs.size()) && places.size() == keys.size() && bad_cus.size() == bad.size();
    for (size_t i = 0; ok && i < keys.size(); ++i) ok = places[i].key() == keys[i];
    for (size_t i = 0; ok && i < bad.size(); ++i) ok = bad_cus[i].where.key() == bad[i].first && bad_cus[i].errors == bad[i].second;
    return ok;
  }
};

// one launch into both; returns CuCoverage's "some workgroup counted errors"
static bool launch(CuCoverage& c, NaiveCoverage& n, const std::vector<uint32_t>& loc, const std::vector<unsigned>& errs) {
  n.locs.push_back(loc);
  n.errs.push_back(errs);
  return c.add(loc, errs);
}

static void test_coverage() {
  const std::vector<unsigned> clean(8, 0);
  {  // cu-check's two words: 8 workgroups on 4 places of 2 XCDs, then 8 on 8, no errors
    CuCoverage c(1);
    NaiveCoverage n{1, {}, {}};
    std::vector<uint32_t> loc;
    for (int b = 0; b < 8; ++b) {
      loc.push_back(hw_word(b & 1, 3, b & 3));
      loc.push_back(b < 4 ? 0 : 5);
    }
    CHECK(!launch(c, n, loc, clean) && c.cus_covered() == 4 && c.xccs() == 2 && c.bad_cus().empty() && n.agrees(c));
    loc.clear();
    for (int b = 0; b < 8; ++b) {
      loc.push_back(hw_word(b, 8, 0));
      loc.push_back(7);
    }
    CuCoverage d(1);
    NaiveCoverage m{1, {}, {}};
    CHECK(!launch(d, m, loc, clean) && d.cus_covered() == 8 && d.xccs() == 1 && m.agrees(d));
    const std::vector<CuLocation> places = d.locations();
    for (size_t i = 0; i + 1 < places.size(); ++i) CHECK(places[i].key() < places[i + 1].key());
  }
  {  // two launches that complete the coverage of 8 CUs between them; errors in two workgroups of one CU add up
    CuCoverage c(1);
    NaiveCoverage n{1, {}, {}};
    std::vector<uint32_t> first, second;
    for (int b = 0; b < 8; ++b) {
      first.push_back(hw_word(0, b % 5, 0));
      first.push_back(1);
      second.push_back(hw_word(0, 3 + b % 5, 0));
      second.push_back(1);
    }
    std::vector<unsigned> errs(8, 0);
    errs[1] = 2;  // CU 1
    errs[6] = 5;  // CU 1 again
    errs[4] = 1;  // CU 4
    CHECK(launch(c, n, first, errs) && c.cus_covered() == 5 && n.agrees(c));
    CHECK(!launch(c, n, second, clean) && c.cus_covered() == 8 && n.agrees(c));
    const std::vector<CuBadCu> bad = c.bad_cus();
    CHECK(bad.size() == 2 && bad[0].where.cu == 1 && bad[0].errors == 7 && bad[1].where.cu == 4 && bad[1].errors == 1);
    errs.assign(8, 0);
    errs[0] = 3;  // CU 3, in a later launch: the counts of a CU accumulate over launches
    CHECK(launch(c, n, second, errs) && n.agrees(c) && c.bad_cus().size() == 3 && c.bad_cus()[1].where.cu == 3);
  }
  {  // more than 16 bad CUs: the first 16 in key order, however they arrived
    CuCoverage c(1);
    NaiveCoverage n{1, {}, {}};
    std::vector<uint32_t> loc;
    std::vector<unsigned> errs;
    for (int b = 39; b >= 0; --b) {
      loc.push_back(hw_word(b / 10, b % 10, 0));
      loc.push_back(b & 1 ? 2 : 9);
      errs.push_back(b + 1);
    }
    CHECK(launch(c, n, loc, errs) && c.cus_covered() == 40 && n.agrees(c));
    const std::vector<CuBadCu> bad = c.bad_cus();
    CHECK(bad.size() == 16 && c.bad_cus(40).size() == 40 && c.bad_cus(3).size() == 3);
    for (size_t i = 0; i + 1 < bad.size(); ++i) CHECK(bad[i].where.key() < bad[i + 1].where.key());
    CHECK(bad[0].where.xcc == 2 && bad[15].where.xcc == 2);  // 20 of the 40 are on XCD 2, which sorts first
  }
  {  // lane-check's 17 words: 16 HW_IDs, then XCC_ID; two waves of a workgroup on one SIMD count once
    CuCoverage c(16);
    NaiveCoverage n{16, {}, {}};
    std::vector<uint32_t> loc;
    for (int b = 0; b < 8; ++b) {  // 4 CUs, two workgroups each: the first covers SIMDs 0..2, the second 1..3
      for (int v = 0; v < 16; ++v) loc.push_back(hw_word(1, b >> 1, (b & 1) + v % 3, v));
      loc.push_back(4);
    }
    std::vector<unsigned> errs(8, 0);
    errs[7] = 9;
    CHECK(launch(c, n, loc, errs) && c.cus_covered() == 4 && c.simds_covered() == 16 && c.xccs() == 1 && n.agrees(c));
    CHECK(c.bad_cus().size() == 1 && c.bad_cus()[0].where.cu == 3 && c.bad_cus()[0].errors == 9);
    CuCoverage part(16);
    NaiveCoverage pn{16, {}, {}};
    loc.resize(17);  // one workgroup alone: 3 SIMDs of one CU
    CHECK(!launch(part, pn, loc, {0}) && part.cus_covered() == 1 && part.simds_covered() == 3 && pn.agrees(part));
  }
}

// ---- the command line
struct Parsed {
  int rc;
  CheckCli cli;
  int units = 0;
  bool flag = false;
  long own = -1;
};

// a program like cu-check and lane-check (a boolean flag, --units), like atomic-check (--units and a flag of
// its own that refuses through bad_arg) or like hbm-check (no --ms, its own bound and default of --rounds)
static Parsed parse_as(const char* prog, std::vector<const char*> args) {
  static const char* const names[3] = {"lds", "valu", "trans"};
  const bool hbm = !std::strcmp(prog, "hbm-check"), atomic = !std::strcmp(prog, "atomic-check");
  Parsed p{0, hbm ? CheckCli{prog, 64, 1000000, false} : CheckCli{prog, atomic ? 64 : 4096}};
  if (hbm) p.cli.rounds = 1;
  args.insert(args.begin(), prog);
  auto value = [&](const char* f, const char* v) {
    if (!hbm && !std::strcmp(f, "--units")) {
      p.units = unit_mask(v, names, 3);
    } else if ((hbm || atomic) && !std::strcmp(f, "--own")) {
      if (!CheckCli::integer(v, &p.own, 2, 10)) return p.cli.bad_arg(f, v);
    } else {
      return CheckCli::unknown;
    }
    return 0;
  };
  char** argv = const_cast<char**>(args.data());
  if (hbm || atomic)
    p.rc = p.cli.parse(static_cast<int>(args.size()), argv, {}, value);
  else
    p.rc = p.cli.parse(static_cast<int>(args.size()), argv, {{"--require-coverage", &p.flag}}, value);
  return p;
}

static void test_cli() {
  for (const char* prog : {"cu-check", "lane-check", "atomic-check", "hbm-check"}) {
    const std::string head = std::string(prog) + ": bad argument ";
    const bool hbm = !std::strcmp(prog, "hbm-check"), atomic = !std::strcmp(prog, "atomic-check");
    auto refused = [&](std::vector<const char*> args, const std::string& line) {
      const Parsed p = parse_as(prog, args);
      return p.rc == 2 && p.cli.err == line + "\n";
    };
    {  // nothing given: the defaults, no message
      const Parsed p = parse_as(prog, {});
      CHECK(p.rc == 0 && p.cli.err.empty() && p.cli.ms == 200 && p.cli.rounds == (hbm ? 1 : 0) && p.cli.device == 0 &&
            p.cli.flips == 0 && p.cli.seed == 0x5eedu && !p.flag);
    }
    {  // every common flag, integers in any base
      const Parsed p = parse_as(prog, {"--rounds", "0x10", "--device", "3", "--seed", "0xdeadbeef", "--selftest-flips", "010"});
      CHECK(p.rc == 0 && p.cli.rounds == 16 && p.cli.device == 3 && p.cli.seed == 0xdeadbeefu && p.cli.flips == 8);
    }
    // a value flag without a value, known or not; an unknown flag with one
    for (const char* f : {"--ms", "--rounds", "--device", "--seed", "--selftest-flips", "--units", "--bogus", "stray"})
      CHECK(refused({f}, head + f + " (missing)"));
    CHECK(refused({"--rounds", "1", "--seed"}, head + "--seed (missing)"));
    CHECK(refused({"--bogus", "1"}, head + "--bogus (unknown flag)"));
    CHECK(refused({"stray", "1"}, head + "stray (unknown flag)"));
    // --ms: the whole string, > 0, so no NaN; hbm-check does not know it
    if (hbm) {
      CHECK(refused({"--ms", "5"}, head + "--ms (unknown flag)"));
    } else {
      for (const char* v : {"0", "-1", "nan", "abc", "5x", ""}) CHECK(refused({"--ms", v}, head + "--ms " + v));
      const Parsed p = parse_as(prog, {"--ms", "1e-3"}), q = parse_as(prog, {"--ms", "inf"});
      CHECK(p.rc == 0 && p.cli.ms == 1e-3 && q.rc == 0 && q.cli.ms > 1e300);
    }
    // --rounds in [1, max]
    const char* over = hbm ? "1000001" : "2000000001";
    for (const char* v : {"0", "-3", over, "1x", "", "99999999999999999999"}) CHECK(refused({"--rounds", v}, head + "--rounds " + v));
    CHECK(parse_as(prog, {"--rounds", hbm ? "1000000" : "2000000000"}).cli.rounds == (hbm ? 1000000 : 2000000000));
    // --device >= 0
    for (const char* v : {"-1", "x", ""}) CHECK(refused({"--device", v}, head + "--device " + v));
    // --seed: the whole string; negative and overflowing values are taken
    for (const char* v : {"zz", "1 ", ""}) CHECK(refused({"--seed", v}, head + "--seed " + v));
    CHECK(parse_as(prog, {"--seed", "-1"}).cli.seed == 0xffffffffu);
    CHECK(parse_as(prog, {"--seed", "99999999999999999999999"}).rc == 0);
    // --selftest-flips in [0, max]
    const char* most = hbm || atomic ? "64" : "4096";
    const char* more = hbm || atomic ? "65" : "4097";
    for (const char* v : {"-1", more, "x"}) CHECK(refused({"--selftest-flips", v}, head + "--selftest-flips " + v));
    CHECK(parse_as(prog, {"--selftest-flips", most}).cli.flips == std::atol(most));
    CHECK(parse_as(prog, {"--selftest-flips", "0"}).rc == 0);
    if (!hbm) {  // --units: the mask, or the list's own message without "bad argument"
      CHECK(parse_as(prog, {"--units", "trans,lds"}).units == 5);
      CHECK(refused({"--units", "lds,foo"}, std::string(prog) + ": unknown unit 'foo': expected a comma list over lds, valu, trans"));
      CHECK(refused({"--units", "lds,"}, std::string(prog) + ": unknown unit '': expected a comma list over lds, valu, trans"));
    } else {
      CHECK(refused({"--units", "lds"}, head + "--units (unknown flag)"));
    }
    if (hbm || atomic) {  // a flag of the program's own, and no boolean flag
      CHECK(parse_as(prog, {"--own", "7"}).own == 7);
      CHECK(refused({"--own", "11"}, head + "--own 11") && refused({"--own"}, head + "--own (missing)"));
      CHECK(refused({"--require-coverage"}, head + "--require-coverage (missing)"));
      CHECK(refused({"--require-coverage", "1"}, head + "--require-coverage (unknown flag)"));
    } else {  // the boolean flag takes no value, wherever it stands
      const Parsed p = parse_as(prog, {"--require-coverage"}), q = parse_as(prog, {"--rounds", "2", "--require-coverage", "--seed", "7"});
      CHECK(p.rc == 0 && p.flag && q.rc == 0 && q.flag && q.cli.rounds == 2 && q.cli.seed == 7);
      CHECK(refused({"--require-coverage", "--ms"}, head + "--ms (missing)"));
      CHECK(refused({"--rounds", "--require-coverage"}, head + "--rounds --require-coverage"));
      CHECK(refused({"--own", "7"}, head + "--own (unknown flag)"));
    }
    {  // the first refusal ends the parse; what a program finds after it goes through the same two calls
      Parsed p = parse_as(prog, {"--rounds", "0", "--bogus", "1"});
      CHECK(p.rc == 2 && p.cli.err == head + "--rounds 0\n");
      CHECK(p.cli.bad_arg("--selftest-flips", "needs one of the units int, fp, ret") == 2 &&
            p.cli.err == head + "--selftest-flips needs one of the units int, fp, ret\n");
      CHECK(p.cli.fail("mib must be at least 2") == 2 && p.cli.err == std::string(prog) + ": mib must be at least 2\n");
    }
  }
}

int main() {
  test_calibrate();
  test_flip_positions();
  test_split_list();
  test_unit_mask();
  test_location();
  test_coverage();
  test_cli();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK check_core: calibrate, flip_positions, split_list, unit_mask, CuLocation, CuCoverage; check_cli: CheckCli\n");
  return 0;
}
