// rocm-vector-add: the GPU-pod validation workload (MI355X replacement for the reference's
// cuda-vector-add test image, test/images/cuda-vector-add/Dockerfile:19-26, run by
// test/e2e/scheduling/nvidia-gpus.go:51-113: success = exit 0 and "Test PASSED").
//
// It runs on whatever GPU the runtime made visible (ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES
// set from the device plugin's InitContainer response) and prints that GPU's identity so
// e2e tests can assert the pod used exactly its assigned device. Flags, output lines and exit
// codes are the contract it shares with hsa-vector-add (vadd_contract.h).
//   rocm-vector-add [-n ELEMENTS] [--print-uuid] [--json] [--expect-devices K]
#include "gpu_common.h"

int main(int argc, char** argv) {
  using namespace amdkube;
  const VaddOptions o = vadd_parse_args(argc, argv);
  try {
    int count = 0;
    AK_HIP(hipGetDeviceCount(&count));
    if (const int rc = vadd_check_device_count(stderr, count, o.expect_devices); rc >= 0) return rc;
    const DevInfo d = dev_info(0);
    const VaddGpu gpu{d.name.c_str(), d.arch.c_str(), d.pci_bus_id.c_str(), d.uuid.c_str(), d.cu_count, count};
    if (o.print_uuid || !o.json) vadd_print_identity(stdout, gpu);
    vadd_print_header(stdout, o.n);
    const VaddResult r = run_vector_add(o.n, 0);
    if (o.json) vadd_print_json(stdout, r.mismatches, o.n, r.kernel_ms, gpu);
    return vadd_print_verdict(stdout, r.mismatches);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "rocm-vector-add: %s\n", e.what());
    return VADD_ERROR;
  }
}
