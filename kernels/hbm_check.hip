// hbm-check: a located march test of the HBM of one MI355X (the device plugin runs it with --hbm-check-mib,
// and it is a GPU-pod workload).
//   hbm-check [--mib M | --free-fraction F] [--chunk-mib C] [--rounds R] [--hold-ms H] [--device D] [--seed S]
//             [--selftest-flips N]
// The region is M MiB (default 1024) or the share F, in (0, 0.95], of the device's free memory, rounded
// down to whole 2 MiB pages and split into chunks of C MiB (default 1024, even). Every round writes an
// address-hashed background, reads it back and writes its complement going up, reads that and writes the
// background going down, and reads it once more (kernels/hbm_check.h), each step over the whole region, with
// a host sleep of H ms between the second and the third. --selftest-flips corrupts N <= 64 slots of the
// region between those two steps of the first round, to prove the check reports them. Prints one JSON line:
// the free memory the region was planned against, the counts, the 2 MiB pages with errors, and the first
// records with the offset, the bits and the XCD / shader engine / CU that read them.
// Exit 0 clean, 1 mismatches, 2 a bad argument or a region that does not fit (the flags are judged before
// anything touches the GPU), 4 a runtime error, out of memory included.
#include "check_cli.h"
#include "hbm_check.h"

using namespace amdkube;

int main(int argc, char** argv) {
  CheckCli cli{"hbm-check", HBM_CHECK_MAX_FLIPS, HBM_CHECK_MAX_ROUNDS, /*takes_ms=*/false};
  cli.rounds = 1;
  long mib = 0, chunk_mib = HBM_CHUNK_MIB_DEFAULT, hold_ms = 0;
  double fraction = 0;
  bool has_mib = false, has_fraction = false;
  if (cli.parse(argc, argv, {}, [&](const char* f, const char* v) {
        if (!std::strcmp(f, "--mib")) {
          if (!CheckCli::integer(v, &mib, 2, HBM_MIB_MAX)) return cli.bad_arg(f, v);
          has_mib = true;
        } else if (!std::strcmp(f, "--free-fraction")) {
          if (!CheckCli::real(v, &fraction) || !(fraction > 0 && fraction <= HBM_FREE_FRACTION_MAX)) return cli.bad_arg(f, v);
          has_fraction = true;
        } else if (!std::strcmp(f, "--chunk-mib")) {
          if (!CheckCli::integer(v, &chunk_mib)) return cli.bad_arg(f, v);
        } else if (!std::strcmp(f, "--hold-ms")) {
          if (!CheckCli::integer(v, &hold_ms, 0, HBM_CHECK_MAX_HOLD_MS)) return cli.bad_arg(f, v);
        } else {
          return CheckCli::unknown;
        }
        return 0;
      }))
    return cli.refuse();
  if (!has_mib && !has_fraction) mib = 1024;
  try {
    hbm_plan_check_args(mib, fraction, chunk_mib);   // both of --mib and --free-fraction, a bad chunk size
  } catch (const std::invalid_argument& e) {
    cli.fail(e.what());
    return cli.refuse();
  }
  return check_run(cli.prog, [&] {
    try {
      const int dev = static_cast<int>(cli.device);
      const DevInfo d = dev_info(dev);
      const unsigned long long free_bytes = hbm_free_bytes(dev);
      const HbmPlan plan = hbm_plan(free_bytes, mib, fraction, chunk_mib);
      const HbmCheckResult r = run_hbm_check(plan, static_cast<int>(cli.rounds), cli.seed, static_cast<int>(cli.flips),
                                             static_cast<int>(hold_ms), dev);
      print_head(dev, d.uuid, d.arch);
      std::printf(",\"free_bytes\":%llu,\"bytes\":%llu,\"chunks\":[", free_bytes, r.bytes);
      for (size_t i = 0; i < r.chunks.size(); ++i) std::printf("%s%llu", i ? "," : "", r.chunks[i]);
      std::printf("],\"rounds\":%d,\"hold_ms\":%d,\"ms\":%.2f,\"alloc_ms\":%.2f,\"march_gbps\":%.1f,\"errors\":%llu,"
                  "\"bit_errors\":%llu,\"transient\":%llu,\"persistent\":%llu,\"records_dropped\":%llu,\"bad_pages_total\":%llu,"
                  "\"bad_pages\":[",
                  r.rounds, r.hold_ms, r.ms, r.alloc_ms, r.march_gbps, r.errors, r.bit_errors, r.transient, r.persistent,
                  r.records_dropped, r.bad_pages_total);
      for (size_t i = 0; i < r.bad_pages.size(); ++i)
        std::printf("%s{\"offset\":%llu,\"chunk\":%u,\"errors\":%u}", i ? "," : "", r.bad_pages[i].offset, r.bad_pages[i].chunk,
                    r.bad_pages[i].errors);
      std::printf("],\"first_errors\":[");
      for (size_t i = 0; i < r.first_errors.size(); ++i) {
        const HbmCheckRecord& e = r.first_errors[i];
        std::printf("%s{\"round\":%u,\"pass\":%u,\"chunk\":%u,\"slot\":%u,\"word\":%u,\"offset\":%llu,\"got\":%u,\"want\":%u,"
                    "\"again\":%u,",
                    i ? "," : "", e.round, e.pass, e.chunk, e.slot, e.word, hbm_region_offset(plan, e.chunk, e.slot) + 4ull * e.word,
                    e.got, e.want, e.again);
        print_location(cu_decode_location(e.hw_id, e.xcc_id));
        std::printf("}");
      }
      std::printf("]}\n");
      return r.errors ? 1 : 0;
    } catch (const std::invalid_argument& e) {   // the region does not fit the free memory
      cli.fail(e.what());
      return cli.refuse();
    }
  });
}
