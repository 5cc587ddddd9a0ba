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
#include "check_cli.h"
#include "lane_check.h"

using namespace amdkube;

int main(int argc, char** argv) {
  CheckCli cli{"lane-check", LANE_MAX_FLIPS};
  int units = LANE_UNIT_ALL;
  bool require_coverage = false;
  if (cli.parse(argc, argv, {{"--require-coverage", &require_coverage}}, [&](const char* f, const char* v) {
        if (std::strcmp(f, "--units")) return CheckCli::unknown;
        units = unit_mask(v, LANE_UNIT_NAMES, 4);
        return 0;
      }))
    return cli.refuse();
  return check_run(cli.prog, [&] {
    const int dev = static_cast<int>(cli.device);
    const DevInfo d = dev_info(dev);
    const LaneCheckResult r = run_lane_check(static_cast<int>(cli.rounds), cli.ms, dev, cli.seed, static_cast<int>(cli.flips), units);
    print_head(dev, d.uuid, d.arch);
    print_units(units, LANE_UNIT_NAMES, 4);
    std::printf(",\"blocks\":%d,\"rounds\":%lld,\"launches\":%d,\"ms\":%.2f,\"xlane_gops\":%.1f,\"tr_gbps\":%.1f,\"dma_gbps\":%.1f,"
                "\"cus\":%d,\"cus_covered\":%d,\"simds\":%d,\"simds_covered\":%d,\"xccs\":%d,\"errors\":%llu,"
                "\"errors_by_unit\":{\"dpp\":%llu,\"perm\":%llu,\"tr\":%llu,\"dma\":%llu}",
                r.blocks, r.rounds, r.launches, r.ms, r.xlane_gops, r.tr_gbps, r.dma_gbps, r.cus, r.cus_covered, r.simds,
                r.simds_covered, r.xccs, r.errors, r.errors_by_unit[0], r.errors_by_unit[1], r.errors_by_unit[2], r.errors_by_unit[3]);
    print_bad_cus(r.bad_cus);
    std::printf(",\"first_errors\":[");
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const LaneCheckRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"block\":%u,", i ? "," : "", LANE_UNIT_NAMES[e.unit < 4 ? e.unit : 0], e.block);
      print_location(cu_decode_location(e.hw_id, e.xcc_id));
      std::printf(",\"simd\":%d,\"round\":%u,\"op\":%u,\"lane\":%u,\"got\":%u,\"want\":%u}", cu_decode_simd(e.hw_id), e.round,
                  e.op, e.lane, e.got, e.want);
    }
    std::printf("]}\n");
    if (r.errors) return 1;
    return require_coverage && (r.cus_covered < r.cus || r.simds_covered < r.simds) ? 1 : 0;
  });
}
