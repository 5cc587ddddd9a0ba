// mfma-check: matrix-core integrity check for one MI355X (device health probe run by the AMD
// device plugin beside hbm-probe, and a GPU-pod workload).
//   mfma-check [--ms D] [--rounds R] [--device D] [--seed S] [--selftest-flips N] [--dtype LIST]
// Every workgroup multiplies hashed integer bf16 tiles with MFMA, checks round 0 against exact
// int32 arithmetic and every later round bitwise against round 0. --rounds runs exactly R rounds,
// otherwise the run is calibrated to ~D ms (default 200). --selftest-flips perturbs N compared
// values to prove the checker reports them. Prints one JSON line; exit 1 on any mismatch.
// --dtype takes a comma list over bf16, fp8, mxfp8 and mxfp4 (the FP8 MFMA and the block-scaled
// e4m3 / e2m1 forms, kernels/mfma_check_lp.h): one JSON line per dtype in the order given, each
// with "dtype" and "tflops", stopping after the first dtype with mismatches; the other flags apply
// to each dtype. Exit 2 on an unknown dtype, 4 on a runtime error.
#include <cstdlib>
#include <cstring>

#include "mfma_check_lp.h"

static void print_errors(const amdkube::MfmaCheckResult& r) {
  std::printf("\"errors\":%llu,\"first_errors\":[", r.errors);
  for (size_t i = 0; i < r.first_errors.size(); ++i) {
    const amdkube::MfmaCheckRecord& e = r.first_errors[i];
    std::printf("%s{\"block\":%u,\"row\":%u,\"col\":%u,\"round\":%u,\"got\":%u,\"want\":%u}", i ? "," : "", e.block, e.row,
                e.col, e.round, e.got, e.want);
  }
  std::printf("]}\n");
}

int main(int argc, char** argv) {
  double ms = 200;
  int rounds = 0, dev = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  const char* dtypes = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--ms") && i + 1 < argc) ms = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) dev = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 0));
    else if (!std::strcmp(argv[i], "--selftest-flips") && i + 1 < argc) flips = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--dtype") && i + 1 < argc) dtypes = argv[++i];
  }
  // without --dtype: the bf16 check, printed without "dtype" and "tflops". Every name is checked before anything runs
  std::vector<int> fmts;
  for (const std::string& name : amdkube::split_list(dtypes ? dtypes : "bf16")) {
    try {
      fmts.push_back(amdkube::mfma_lp_fmt(name, amdkube::MFMA_BF16));
    } catch (const std::invalid_argument&) {
      std::fprintf(stderr, "mfma-check: unknown dtype '%s': expected a comma list over bf16, fp8, mxfp8, mxfp4\n",
                   name.c_str());
      return 2;
    }
  }
  try {
    amdkube::DevInfo d = amdkube::dev_info(dev);
    for (int f : fmts) {
      amdkube::MfmaCheckResult r = amdkube::run_mfma_check_lp(f, rounds, ms, dev, seed, flips);
      std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",", dev, d.uuid.c_str(), d.arch.c_str());
      if (dtypes) std::printf("\"dtype\":\"%s\",", amdkube::mfma_lp_name(f));
      std::printf("\"blocks\":%d,\"rounds\":%lld,\"k\":%d,\"ms\":%.2f,", r.blocks, r.rounds, r.k, r.ms);
      if (f == amdkube::MFMA_BF16) std::printf("\"bf16_tflops\":%.1f,", r.tflops);
      if (dtypes) std::printf("\"tflops\":%.1f,", r.tflops);
      print_errors(r);
      std::fflush(stdout);
      if (r.errors) return 1;  // the failing line is the last one printed
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mfma-check: %s\n", e.what());
    return 4;
  }
}
