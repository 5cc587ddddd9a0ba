// mfma-check: matrix-core integrity check for one MI355X (device health probe run by the AMD
// device plugin beside hbm-probe, and a GPU-pod workload).
//   mfma-check [--ms D] [--rounds R] [--device D] [--seed S] [--selftest-flips N]
// Every workgroup multiplies hashed integer bf16 tiles with MFMA, checks round 0 against exact
// int32 arithmetic and every later round bitwise against round 0. --rounds runs exactly R rounds,
// otherwise the run is calibrated to ~D ms (default 200). --selftest-flips perturbs N compared
// values to prove the checker reports them. Prints one JSON line; exit 1 on any mismatch.
#include <cstdlib>
#include <cstring>

#include "gpu_common.h"

int main(int argc, char** argv) {
  double ms = 200;
  int rounds = 0, dev = 0, flips = 0;
  uint32_t seed = 0x5eedu;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--ms") && i + 1 < argc) ms = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--rounds") && i + 1 < argc) rounds = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) dev = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--seed") && i + 1 < argc) seed = static_cast<uint32_t>(std::strtoul(argv[++i], nullptr, 0));
    else if (!std::strcmp(argv[i], "--selftest-flips") && i + 1 < argc) flips = std::atoi(argv[++i]);
  }
  try {
    amdkube::DevInfo d = amdkube::dev_info(dev);
    amdkube::MfmaCheckResult r = amdkube::run_mfma_check(rounds, ms, dev, seed, flips);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"arch\":\"%s\",\"blocks\":%d,\"rounds\":%lld,\"k\":%d,\"ms\":%.2f,"
                "\"bf16_tflops\":%.1f,\"errors\":%llu,\"first_errors\":[",
                dev, d.uuid.c_str(), d.arch.c_str(), r.blocks, r.rounds, r.k, r.ms, r.tflops, r.errors);
    for (size_t i = 0; i < r.first_errors.size(); ++i) {
      const amdkube::MfmaCheckRecord& e = r.first_errors[i];
      std::printf("%s{\"block\":%u,\"row\":%u,\"col\":%u,\"round\":%u,\"got\":%u,\"want\":%u}", i ? "," : "", e.block, e.row,
                  e.col, e.round, e.got, e.want);
    }
    std::printf("]}\n");
    return r.errors ? 1 : 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mfma-check: %s\n", e.what());
    return 4;
  }
}
