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
#include "atomic_check.h"
#include "check_cli.h"

using namespace amdkube;

int main(int argc, char** argv) {
  CheckCli cli{"atomic-check", ATOMIC_MAX_FLIPS};
  int units = ATOMIC_UNIT_ALL;
  std::vector<uint32_t> contention = atomic_default_contention();
  const int blocks = ATOMIC_DEFAULT_BLOCKS;
  if (cli.parse(argc, argv, {}, [&](const char* f, const char* v) {
        if (!std::strcmp(f, "--units")) {
          units = unit_mask(v, ATOMIC_UNIT_NAMES, 4);
        } else if (!std::strcmp(f, "--contention")) {
          contention = atomic_check_contention(v);
          for (uint32_t c : contention)
            if (c > static_cast<uint32_t>(blocks) * ATOMIC_WG) return cli.bad_arg(f, v);
        } else {
          return CheckCli::unknown;
        }
        return 0;
      }))
    return cli.refuse();
  if (cli.flips > 0 && !(units & ~ATOMIC_UNIT_LDS)) {
    cli.bad_arg("--selftest-flips", "needs one of the units int, fp, ret");
    return cli.refuse();
  }
  return check_run(cli.prog, [&] {
    const int dev = static_cast<int>(cli.device);
    const DevInfo d = dev_info(dev);
    const AtomicCheckResult r = run_atomic_check(static_cast<int>(cli.rounds), cli.ms, dev, cli.seed, static_cast<int>(cli.flips),
                                                 units, contention, blocks);
    print_head(dev, d.uuid, d.arch);
    print_units(units, ATOMIC_UNIT_NAMES, 4);
    std::printf(",\"contention\":[");
    for (size_t i = 0; i < r.contention.size(); ++i) std::printf("%s%u", i ? "," : "", r.contention[i]);
    std::printf("],\"blocks\":%d,\"rounds\":%lld,\"ms\":%.2f,\"checked\":%llu,\"atomics_per_s\":%.4g,\"errors\":%llu,"
                "\"errors_by_unit\":{\"int\":%llu,\"fp\":%llu,\"ret\":%llu,\"lds\":%llu},\"first_errors\":[",
                r.blocks, r.rounds, r.ms, r.checked, r.atomics_per_s, r.errors, r.errors_by_unit[0], r.errors_by_unit[1],
                r.errors_by_unit[2], r.errors_by_unit[3]);
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const AtomicRecord& e = r.first_errors[i];
      std::printf("%s{\"unit\":\"%s\",\"op\":\"%s\",\"slot\":%u,\"round\":%u,\"contention\":%u,\"offset\":%u,"
                  "\"got\":[%u,%u],\"want\":[%u,%u]",
                  i ? "," : "", ATOMIC_UNIT_NAMES[e.unit < 4 ? e.unit : 0], ATOMIC_OP_NAMES[e.op < AOP_COUNT ? e.op : 0], e.slot,
                  e.round, e.contention, e.offset, e.got_lo, e.got_hi, e.want_lo, e.want_hi);
      if (e.unit == 3) {   // an LDS atomic fault belongs to a CU
        std::printf(",");
        print_location(cu_decode_location(e.hw_id, e.xcc_id));
      }
      std::printf("}");
    }
    std::printf("]}\n");
    return r.errors ? 1 : 0;
  });
}
