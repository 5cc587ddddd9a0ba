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
#include <cstdlib>
#include <cstring>

#include "hbm_check.h"

int main(int argc, char** argv) {
  long mib = 0, chunk_mib = amdkube::HBM_CHUNK_MIB_DEFAULT, rounds = 1, hold_ms = 0, dev = 0, flips = 0;
  double fraction = 0;
  bool has_mib = false, has_fraction = false;
  uint32_t seed = 0x5eedu;
  auto bad_arg = [](const char* what, const char* v) {
    std::fprintf(stderr, "hbm-check: bad argument %s %s\n", what, v ? v : "(missing)");
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
    if (!std::strcmp(f, "--mib")) {
      if (!integer(v, &mib) || mib < 2 || mib > amdkube::HBM_MIB_MAX) return bad_arg(f, v);
      has_mib = true;
    } else if (!std::strcmp(f, "--free-fraction")) {
      char* end = nullptr;
      fraction = std::strtod(v, &end);
      if (end == v || *end || !(fraction > 0 && fraction <= amdkube::HBM_FREE_FRACTION_MAX)) return bad_arg(f, v);
      has_fraction = true;
    } else if (!std::strcmp(f, "--chunk-mib")) {
      if (!integer(v, &chunk_mib)) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--rounds")) {
      if (!integer(v, &rounds) || rounds < 1 || rounds > amdkube::HBM_CHECK_MAX_ROUNDS) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--hold-ms")) {
      if (!integer(v, &hold_ms) || hold_ms < 0 || hold_ms > amdkube::HBM_CHECK_MAX_HOLD_MS) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--device")) {
      if (!integer(v, &dev) || dev < 0) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--seed")) {
      char* end = nullptr;
      seed = static_cast<uint32_t>(std::strtoul(v, &end, 0));
      if (end == v || *end) return bad_arg(f, v);
    } else if (!std::strcmp(f, "--selftest-flips")) {
      if (!integer(v, &flips) || flips < 0 || flips > amdkube::HBM_CHECK_MAX_FLIPS) return bad_arg(f, v);
    } else {
      return bad_arg(f, "(unknown flag)");
    }
  }
  if (!has_mib && !has_fraction) mib = 1024;
  try {
    amdkube::hbm_plan_check_args(mib, fraction, chunk_mib);   // both of --mib and --free-fraction, a bad chunk size
  } catch (const std::invalid_argument& e) {
    std::fprintf(stderr, "hbm-check: %s\n", e.what());
    return 2;
  }
  try {
    const int d_ = static_cast<int>(dev);
    const amdkube::DevInfo d = amdkube::dev_info(d_);
    const unsigned long long free_bytes = amdkube::hbm_free_bytes(d_);
    const amdkube::HbmPlan plan = amdkube::hbm_plan(free_bytes, mib, fraction, chunk_mib);
    const amdkube::HbmCheckResult r =
        amdkube::run_hbm_check(plan, static_cast<int>(rounds), seed, static_cast<int>(flips), static_cast<int>(hold_ms), d_);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",\"free_bytes\":%llu,\"bytes\":%llu,\"chunks\":[", d_,
                d.uuid.c_str(), d.arch.c_str(), free_bytes, r.bytes);
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
      const amdkube::HbmCheckRecord& e = r.first_errors[i];
      const amdkube::CuLocation l = amdkube::cu_decode_location(e.hw_id, e.xcc_id);
      std::printf("%s{\"round\":%u,\"pass\":%u,\"chunk\":%u,\"slot\":%u,\"word\":%u,\"offset\":%llu,\"got\":%u,\"want\":%u,"
                  "\"again\":%u,\"xcc\":%d,\"se\":%d,\"sh\":%d,\"cu\":%d}",
                  i ? "," : "", e.round, e.pass, e.chunk, e.slot, e.word, amdkube::hbm_region_offset(plan, e.chunk, e.slot) + 4ull * e.word,
                  e.got, e.want, e.again, l.xcc, l.se, l.sh, l.cu);
    }
    std::printf("]}\n");
    return r.errors ? 1 : 0;
  } catch (const std::invalid_argument& e) {   // the region does not fit the free memory
    std::fprintf(stderr, "hbm-check: %s\n", e.what());
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hbm-check: %s\n", e.what());
    return 4;
  }
}
