// lane-check: integrity check of the cross-lane, LDS-transpose and direct-to-LDS data paths of one MI355X
// (run by the AMD device plugin with --lane-check-ms, and a GPU-pod workload).
//   lane-check [--ms D] [--rounds R] [--device D] [--seed S] [--selftest-flips N] [--units LIST] [--require-coverage]
// Every workgroup owns a whole CU's LDS and, round after round, runs every DPP control, the lane swaps and
// v_readlane (dpp), ds_bpermute / ds_permute / ds_swizzle (perm), the four transposing LDS reads (tr) and a
// sweep of its LDS by global_load_lds in all three widths (dma), and compares every result with the value
// worked out from the lane id (kernels/lane_check.h, kernels/lane_plan.h). --units takes a comma list over dpp,
// perm, tr and dma (default: all four). --rounds runs exactly R rounds, otherwise the run is calibrated to
// ~D ms (default 200). --selftest-flips perturbs N compared values to prove the checker reports them. Prints
// one JSON line with the rates, the coverage (cus, cus_covered, simds, simds_covered, xccs), the error counts
// per unit and per CU, and the first records with their XCD / shader engine / CU / SIMD.
// Exit 0 clean (incomplete coverage is reported, and fails only with --require-coverage: exit 1),
// 1 mismatches, 2 an unknown unit or a bad argument (decided before anything touches the GPU),
// 4 a runtime error.
#include <cstdlib>
#include <cstring>

#include "lane_check.h"

static void print_location(const amdkube::CuLocation& l) {
  std::printf("\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d", l.xcc, l.se, l.sh, l.cu);
}

int main(int argc, char** argv) {
  double ms = 200;
  long rounds = 0, dev = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  int units = amdkube::LANE_UNIT_ALL;
  bool require_coverage = false;
  auto bad_arg = [](const char* what, const char* v) {
    std::fprintf(stderr, "lane-check: bad argument %s %s\n", what, v ? v : "(missing)");
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
      if (!integer(v, &flips) || flips < 0 || flips > amdkube::LANE_MAX_FLIPS) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--units")) {
      try {
        units = amdkube::lane_check_units(v);
      } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "lane-check: %s\n", e.what());
        return 2;
      }
    } else {
      return bad_arg(f, "(unknown flag)");
    }
  }
  try {
    const int d_ = static_cast<int>(dev);
    amdkube::DevInfo d = amdkube::dev_info(d_);
    amdkube::LaneCheckResult r =
        amdkube::run_lane_check(static_cast<int>(rounds), ms, d_, seed, static_cast<int>(flips), units);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",\"units\":[", d_, d.uuid.c_str(), d.arch.c_str());
    bool first = true;
    for (int u = 0; u < 4; ++u)
      if (units & (1 << u)) {
        std::printf("%s\"%s\"", first ? "" : ",", amdkube::LANE_UNIT_NAMES[u]);
        first = false;
      }
    std::printf("],\"blocks\":%d,\"rounds\":%lld,\"launches\":%d,\"ms\":%.2f,\"xlane_gops\":%.1f,\"tr_gbps\":%.1f,\"dma_gbps\":%.1f,"
                "\"cus\":%d,\"cus_covered\":%d,\"simds\":%d,\"simds_covered\":%d,\"xccs\":%d,\"errors\":%llu,"
                "\"errors_by_unit\":{\"dpp\":%llu,\"perm\":%llu,\"tr\":%llu,\"dma\":%llu},\"bad_cus\":[",
                r.blocks, r.rounds, r.launches, r.ms, r.xlane_gops, r.tr_gbps, r.dma_gbps, r.cus, r.cus_covered, r.simds,
                r.simds_covered, r.xccs, r.errors, r.errors_by_unit[0], r.errors_by_unit[1], r.errors_by_unit[2], r.errors_by_unit[3]);
    for (size_t i = 0; i < r.bad_cus.size(); ++i) {
      std::printf("%s{", i ? "," : "");
      print_location(r.bad_cus[i].where);
      std::printf(",\"errors\":%llu}", r.bad_cus[i].errors);
    }
    std::printf("],\"first_errors\":[");
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const amdkube::LaneCheckRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"block\":%u,", i ? "," : "", amdkube::LANE_UNIT_NAMES[e.unit < 4 ? e.unit : 0], e.block);
      print_location(amdkube::cu_decode_location(e.hw_id, e.xcc_id));
      std::printf(",\"simd\":%d,\"round\":%u,\"op\":%u,\"lane\":%u,\"got\":%u,\"want\":%u}", amdkube::lane_simd_of(e.hw_id), e.round,
                  e.op, e.lane, e.got, e.want);
    }
    std::printf("]}\n");
    if (r.errors) return 1;
    return require_coverage && (r.cus_covered < r.cus || r.simds_covered < r.simds) ? 1 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "lane-check: %s\n", e.what());
    return 4;
  }
}
