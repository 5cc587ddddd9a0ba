// gpu-burn: synthetic matrix-core load for GPU pods (density / exporter validation).
//   gpu-burn [--ms DURATION] [--device D] [--verify]
// Runs register-resident bf16 MFMA chains on every CU for ~DURATION ms, prints achieved TF.
// --verify runs the checked workload of mfma-check instead (every result compared, see
// mfma_check.h), adds "verified" and "errors" to the JSON and exits 1 on a mismatch.
#include <cstdlib>
#include <cstring>

#include "mfma_check.h"

int main(int argc, char** argv) {
  double ms = 200;
  int dev = 0;
  bool verify = false;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--ms") && i + 1 < argc) ms = std::atof(argv[++i]);
    else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) dev = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--verify")) verify = true;
  }
  try {
    amdkube::DevInfo d = amdkube::dev_info(dev);
    if (verify) {
      amdkube::MfmaCheckResult r = amdkube::run_mfma_check(0, ms, dev);
      std::printf("{\"device\":%d,\"uuid\":\"%s\",\"ms\":%.2f,\"iters\":%lld,\"blocks\":%d,\"bf16_tflops\":%.1f,"
                  "\"verified\":true,\"errors\":%llu}\n",
                  dev, d.uuid.c_str(), r.ms, r.rounds, r.blocks, r.tflops, r.errors);
      return r.errors ? 1 : 0;
    }
    amdkube::BurnResult r = amdkube::run_mfma_burn(ms, dev);
    std::printf("{\"device\":%d,\"uuid\":\"%s\",\"ms\":%.2f,\"iters\":%lld,\"blocks\":%d,\"bf16_tflops\":%.1f}\n", dev,
                d.uuid.c_str(), r.ms, r.iters, r.blocks, r.tflops);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gpu-burn: %s\n", e.what());
    return 4;
  }
}
