// atomic-check: atomic-unit integrity check for one MI355X (run by the AMD device plugin with
// --atomic-check-ms, and a GPU-pod workload).
//   atomic-check [--ms D] [--rounds R] [--device D] [--seed S] [--selftest-flips N] [--units LIST] [--contention LIST]
// Round after round and contention level after level, every lane scatters hashed operands through the
// global atomic ALUs (integer, floating-point and packed ops, a ticket counter and a compare-and-swap loop)
// and the LDS atomic ALU of its CU into tables whose result does not depend on the arrival order, and a
// second kernel recomputes every slot without atomics and compares (kernels/atomic_check.h). --units takes a
// comma list over int, fp, ret and lds (default: all four), --contention a comma list of powers of two
// (lanes per slot; default 1,64,4096). --rounds runs exactly R rounds, otherwise the run is calibrated to
// ~D ms (default 200). --selftest-flips flips one bit of N table slots between scatter and verify to prove
// the verifier reports them. Prints one JSON line.
// Exit 0 clean, 1 mismatches, 2 a bad argument (decided before anything touches the GPU), 4 a runtime error.
#include <cstdlib>
#include <cstring>

#include "atomic_check.h"

int main(int argc, char** argv) {
  double ms = 200;
  long rounds = 0, dev = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  int units = amdkube::ATOMIC_UNIT_ALL;
  std::vector<uint32_t> contention = amdkube::atomic_default_contention();
  const int blocks = amdkube::ATOMIC_DEFAULT_BLOCKS;
  auto bad_arg = [](const char* what, const char* v) {
    std::fprintf(stderr, "atomic-check: bad argument %s %s\n", what, v ? v : "(missing)");
    return 2;
  };
  auto integer = [](const char* s, long* out) {
    char* end = nullptr;
    *out = std::strtol(s, &end, 0);
    return end != s && *end == 0;
  };
  for (int i = 1; i < argc; ++i) {
    const char* f = argv[i];
    const char* v = i + 1 < argc ? argv[++i] : nullptr;
    if (!v) return bad_arg(f, v);
    try {
      if (!std::strcmp(f, "--ms")) {
        char* end = nullptr;
        ms = std::strtod(v, &end);
        if (end == v || *end || !(ms > 0)) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--rounds")) {
        if (!integer(v, &rounds) || rounds < 1 || rounds > 2000000000) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--device")) {
        if (!integer(v, &dev) || dev < 0) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--seed")) {
        char* end = nullptr;
        seed = static_cast<uint32_t>(std::strtoul(v, &end, 0));
        if (end == v || *end) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--selftest-flips")) {
        if (!integer(v, &flips) || flips < 0 || flips > amdkube::ATOMIC_MAX_FLIPS) return bad_arg(f, v);
      } else if (!std::strcmp(f, "--units")) {
        units = amdkube::atomic_check_units(v);
      } else if (!std::strcmp(f, "--contention")) {
        contention = amdkube::atomic_check_contention(v);
        for (uint32_t c : contention)
          if (c > static_cast<uint32_t>(blocks) * amdkube::ATOMIC_WG) return bad_arg(f, v);
      } else {
        return bad_arg(f, "(unknown flag)");
      }
    } catch (const std::invalid_argument& e) {
      std::fprintf(stderr, "atomic-check: %s\n", e.what());
      return 2;
    }
  }
  if (flips > 0 && !(units & ~amdkube::ATOMIC_UNIT_LDS)) return bad_arg("--selftest-flips", "needs one of the units int, fp, ret");
  try {
    const int d_ = static_cast<int>(dev);
    amdkube::DevInfo d = amdkube::dev_info(d_);
    amdkube::AtomicCheckResult r =
        amdkube::run_atomic_check(static_cast<int>(rounds), ms, d_, seed, static_cast<int>(flips), units, contention, blocks);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",\"units\":[", d_, d.uuid.c_str(), d.arch.c_str());
    bool first = true;
    for (int u = 0; u < 4; ++u)
      if (units & (1 << u)) {
        std::printf("%s\"%s\"", first ? "" : ",", amdkube::ATOMIC_UNIT_NAMES[u]);
        first = false;
      }
    std::printf("],\"contention\":[");
    for (size_t i = 0; i < r.contention.size(); ++i) std::printf("%s%u", i ? "," : "", r.contention[i]);
    std::printf("],\"blocks\":%d,\"rounds\":%lld,\"ms\":%.2f,\"checked\":%llu,\"atomics_per_s\":%.4g,\"errors\":%llu,"
                "\"errors_by_unit\":{\"int\":%llu,\"fp\":%llu,\"ret\":%llu,\"lds\":%llu},\"first_errors\":[",
                r.blocks, r.rounds, r.ms, r.checked, r.atomics_per_s, r.errors, r.errors_by_unit[0], r.errors_by_unit[1],
                r.errors_by_unit[2], r.errors_by_unit[3]);
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const amdkube::AtomicRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"op\":\"%s\",\"slot\":%u,\"round\":%u,\"contention\":%u,\"offset\":%u,"
                  "\"got\":[%u,%u],\"want\":[%u,%u]",
                  i ? "," : "", amdkube::ATOMIC_UNIT_NAMES[e.unit < 4 ? e.unit : 0],
                  amdkube::ATOMIC_OP_NAMES[e.op < amdkube::AOP_COUNT ? e.op : 0], e.slot, e.round, e.contention, e.offset, e.got_lo,
                  e.got_hi, e.want_lo, e.want_hi);
      if (e.unit == 3) {   // an LDS atomic fault belongs to a CU
        const amdkube::CuLocation l = amdkube::cu_decode_location(e.hw_id, e.xcc_id);
        std::printf(",\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d", l.xcc, l.se, l.sh, l.cu);
      }
      std::printf("}");
    }
    std::printf("]}\n");
    return r.errors ? 1 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "atomic-check: %s\n", e.what());
    return 4;
  }
}
