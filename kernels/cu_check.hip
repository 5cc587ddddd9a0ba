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
#include "check_cli.h"
#include "cu_check.h"

using namespace amdkube;

int main(int argc, char** argv) {
  CheckCli cli{"cu-check", CU_CHECK_MAX_FLIPS};
  int units = CU_UNIT_ALL;
  bool require_coverage = false;
  if (cli.parse(argc, argv, {{"--require-coverage", &require_coverage}}, [&](const char* f, const char* v) {
        if (std::strcmp(f, "--units")) return CheckCli::unknown;
        units = unit_mask(v, CU_UNIT_NAMES, 3);
        return 0;
      }))
    return cli.refuse();
  return check_run(cli.prog, [&] {
    const int dev = static_cast<int>(cli.device);
    const DevInfo d = dev_info(dev);
    const CuCheckResult r = run_cu_check(static_cast<int>(cli.rounds), cli.ms, dev, cli.seed, static_cast<int>(cli.flips), units);
    print_head(dev, d.uuid, d.arch);
    print_units(units, CU_UNIT_NAMES, 3);
    std::printf(",\"blocks\":%d,\"rounds\":%lld,\"launches\":%d,\"ms\":%.2f,\"lds_gbps\":%.1f,\"valu_gops\":%.1f,"
                "\"cus\":%d,\"cus_covered\":%d,\"xccs\":%d,\"errors\":%llu,\"errors_by_unit\":{\"lds\":%llu,\"valu\":%llu,"
                "\"trans\":%llu}",
                r.blocks, r.rounds, r.launches, r.ms, r.lds_gbps, r.valu_gops, r.cus, r.cus_covered, r.xccs, r.errors,
                r.errors_by_unit[0], r.errors_by_unit[1], r.errors_by_unit[2]);
    print_bad_cus(r.bad_cus);
    std::printf(",\"first_errors\":[");
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const CuCheckRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"block\":%u,", i ? "," : "", CU_UNIT_NAMES[e.unit < 3 ? e.unit : 0], e.block);
      print_location(cu_decode_location(e.hw_id, e.xcc_id));
      std::printf(",\"round\":%u,\"pass\":%u,\"index\":%u,\"got\":%u,\"want\":%u}", e.round, e.pass, e.index, e.got, e.want);
    }
    std::printf("]}\n");
    if (r.errors) return 1;
    return require_coverage && r.cus_covered < r.cus ? 3 : 0;
  });
}
