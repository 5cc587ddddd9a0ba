// cu-check: per-CU integrity check for one MI355X (device health probe run by the AMD device
// plugin after hbm-probe and mfma-check, and a GPU-pod workload).
//   cu-check [--ms D] [--rounds R] [--device D] [--seed S] [--selftest-flips N] [--units LIST] [--require-coverage]
// Every workgroup owns a whole CU's LDS and, round after round, marches all 160 KiB of it, computes the
// same multiply-adds on the fp32, packed-fp32, fp64 and integer pipes and compares them, and runs the
// transcendental unit on two waves that must agree (kernels/cu_check.h). --units takes a comma list
// over lds, valu and trans (default: all three). --rounds runs exactly R rounds, otherwise the run is
// calibrated to ~D ms (default 200). --selftest-flips perturbs N compared values to prove the checker
// reports them. Prints one JSON line with the coverage (cus, cus_covered, xccs), the error counts per
// unit and per CU, and the first records with their XCD / shader engine / CU.
// Exit 0 clean (incomplete coverage is reported, and fails only with --require-coverage: exit 3),
// 1 mismatches, 2 an unknown unit or a bad argument (decided before anything touches the GPU),
// 4 a runtime error.
#include <cstdlib>
#include <cstring>

#include "cu_check.h"

static void print_location(const amdkube::CuLocation& l) {
  std::printf("\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d", l.xcc, l.se, l.sh, l.cu);
}

int main(int argc, char** argv) {
  double ms = 200;
  long rounds = 0, dev = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  int units = amdkube::CU_UNIT_ALL;
  bool require_coverage = false;
  auto bad_arg = [](const char* what, const char* v) {
    std::fprintf(stderr, "cu-check: bad argument %s %s\n", what, v ? v : "(missing)");
    return 2;
  };
  auto integer = [](const char* s, long* out) {
    char* end = nullptr;
    *out = std::strtol(s, &end, 0);
    return end != s && *end == 0;
  };
  for (int i = 1; i < argc; ++i) {
    const char* f = argv[i];
    if (!std::strcmp(f, "--require-coverage")) {
      require_coverage = true;
      continue;
    }
    const char* v = i + 1 < argc ? argv[++i] : nullptr;
    if (!v) return bad_arg(f, v);
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
      if (!integer(v, &flips) || flips < 0 || flips > amdkube::CU_CHECK_MAX_FLIPS) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--units")) {
      try {
        units = amdkube::cu_check_units(v);
      } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "cu-check: %s\n", e.what());
        return 2;
      }
    } else {
      return bad_arg(f, "(unknown flag)");
    }
  }
  try {
    const int d_ = static_cast<int>(dev);
    amdkube::DevInfo d = amdkube::dev_info(d_);
    amdkube::CuCheckResult r =
        amdkube::run_cu_check(static_cast<int>(rounds), ms, d_, seed, static_cast<int>(flips), units);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",\"units\":[", d_, d.uuid.c_str(), d.arch.c_str());
    bool first = true;
    for (int u = 0; u < 3; ++u)
      if (units & (1 << u)) {
        std::printf("%s\"%s\"", first ? "" : ",", amdkube::CU_UNIT_NAMES[u]);
        first = false;
      }
    std::printf("],\"blocks\":%d,\"rounds\":%lld,\"launches\":%d,\"ms\":%.2f,\"lds_gbps\":%.1f,\"valu_gops\":%.1f,"
                "\"cus\":%d,\"cus_covered\":%d,\"xccs\":%d,\"errors\":%llu,\"errors_by_unit\":{\"lds\":%llu,\"valu\":%llu,"
                "\"trans\":%llu},\"bad_cus\":[",
                r.blocks, r.rounds, r.launches, r.ms, r.lds_gbps, r.valu_gops, r.cus, r.cus_covered, r.xccs, r.errors,
                r.errors_by_unit[0], r.errors_by_unit[1], r.errors_by_unit[2]);
    for (size_t i = 0; i < r.bad_cus.size(); ++i) {
      std::printf("%s{", i ? "," : "");
      print_location(r.bad_cus[i].where);
      std::printf(",\"errors\":%llu}", r.bad_cus[i].errors);
    }
    std::printf("],\"first_errors\":[");
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const amdkube::CuCheckRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"block\":%u,", i ? "," : "", amdkube::CU_UNIT_NAMES[e.unit < 3 ? e.unit : 0], e.block);
      print_location(amdkube::cu_decode_location(e.hw_id, e.xcc_id));
      std::printf(",\"round\":%u,\"pass\":%u,\"index\":%u,\"got\":%u,\"want\":%u}", e.round, e.pass, e.index, e.got, e.want);
    }
    std::printf("]}\n");
    if (r.errors) return 1;
    return require_coverage && r.cus_covered < r.cus ? 3 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cu-check: %s\n", e.what());
    return 4;
  }
}
