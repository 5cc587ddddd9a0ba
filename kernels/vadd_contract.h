// The GPU-pod workload's contract, shared by rocm-vector-add (kernels/vector_add.hip, run_vector_add in
// gpu_common.h) and hsa-vector-add (kernels/hsa_vector_add.cpp): the e2e tests, the device-guard tests
// and bench.py --dump-outputs treat the two as one program, so the flags, the input data, the
// verification, the grid, the output lines and the exit codes are written once, here. Plain C++17 with
// no HIP and no HSA in it (kernels/vadd_kernel.hip includes it for VADD_WG); self-tested on the CPU by
// native/vadd_contract_selftest.cpp.
//
// What differs between the two programs stays with them: the "-n 0" message, the "(hsa_init: ...)"
// detail on the HSA no-GPU line, the JSON tail of the HSA build, and the item count each passes to
// stream_grid (HIP rounds the 16-byte words up, HSA down; they differ at n = 1025, for example).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace amdkube {

// ---------------------------------------------------------------------------- work-group size and grid
constexpr unsigned VADD_WG = 256;          // lanes per work-group: the kernels' launch bounds and every launch
constexpr int VADD_BLOCKS_PER_CU = 64;     // the vector add's cap (gpu_common.h, vadd_kernel, says why 64)

// The streaming grid: one work-group per 256 items, at least one, at most per_cu for each CU.
inline int stream_grid(size_t items, int cu_count, int per_cu = 8) {
  size_t want = (items + 255) / 256;
  size_t cap = static_cast<size_t>(cu_count > 0 ? cu_count : 256) * per_cu;
  if (want < 1) want = 1;
  return static_cast<int>(want < cap ? want : cap);
}

// ---------------------------------------------------------------------------- options
struct VaddOptions {
  size_t n = 50000;
  bool print_uuid = false, json = false;
  int expect_devices = -1;                       // < 0: any number
  bool fast_exit = false, no_prefetch = false;   // hsa-vector-add only
};

// Lax on purpose, as the pods' command lines have always been read: strtoull / atoi, an unknown flag
// is ignored, and so is a value flag that is the last argument. Opens nothing and calls no runtime.
inline VaddOptions vadd_parse_args(int argc, char** argv) {
  VaddOptions o;
  for (int i = 1; i < argc; ++i)   // seen wherever it stands, even where a value flag takes it as its value
    if (!std::strcmp(argv[i], "--no-prefetch")) o.no_prefetch = true;
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if ((!std::strcmp(a, "-n") || !std::strcmp(a, "--elements")) && i + 1 < argc) o.n = std::strtoull(argv[++i], nullptr, 10);
    else if (!std::strcmp(a, "--print-uuid")) o.print_uuid = true;
    else if (!std::strcmp(a, "--json")) o.json = true;
    else if (!std::strcmp(a, "--expect-devices") && i + 1 < argc) o.expect_devices = std::atoi(argv[++i]);
    else if (!std::strcmp(a, "--fast-exit")) o.fast_exit = true;
  }
  return o;
}

// ---------------------------------------------------------------------------- inputs and verification
// a[i], b[i] in [0, 1): one LCG, seed 12345, two draws per element.
inline void vadd_fill_inputs(float* a, float* b, size_t n) {
  uint32_t s = 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    a[i] = static_cast<float>(s >> 8) / 16777216.0f;
    s = s * 1664525u + 1013904223u;
    b[i] = static_cast<float>(s >> 8) / 16777216.0f;
  }
}

// Elements of c that are not within 1e-5 of a + b, in float arithmetic. Written as "unless inside the
// bound", so a difference that is NaN counts: a NaN in c (both programs fill c with 0xff bytes before the
// run, so an element the GPU never wrote is one), a NaN input, inf - inf. For every other difference the
// answer is that of the two loops this replaced (native/vadd_contract_selftest.cpp holds all three together).
inline size_t vadd_count_mismatches(const float* a, const float* b, const float* c, size_t n) {
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    const float d = c[i] - (a[i] + b[i]);
    if (!(d <= 1e-5f && d >= -1e-5f)) ++bad;
  }
  return bad;
}

// ---------------------------------------------------------------------------- exit codes and output lines
enum VaddExit { VADD_PASSED = 0, VADD_MISMATCHES = 1, VADD_NO_GPU = 2, VADD_WRONG_DEVICE_COUNT = 3, VADD_ERROR = 4 };

constexpr const char* VADD_FALLBACK_NAME = "AMD Instinct GPU";   // the marketing name needs libdrm's amdgpu.ids on the host

struct VaddGpu {   // the visible GPU the pod ran on; the strings belong to the caller
  const char *product, *arch, *bus, *uuid;
  int cus, visible;
};

// `detail` (HSA: why hsa_init failed) follows the text in parentheses.
inline int vadd_print_no_gpu(FILE* err, const char* detail = nullptr) {
  std::fprintf(err, "no GPU visible to this container%s%s%s\n", detail ? " (" : "", detail ? detail : "", detail ? ")" : "");
  return VADD_NO_GPU;
}

// The device-count checks both programs make first: the exit code to leave with, or -1 to go on.
inline int vadd_check_device_count(FILE* err, int found, int expect) {
  if (found < 1) return vadd_print_no_gpu(err);
  if (expect >= 0 && found != expect) {
    std::fprintf(err, "expected %d visible GPU(s), found %d\n", expect, found);
    return VADD_WRONG_DEVICE_COUNT;
  }
  return -1;
}

inline void vadd_print_identity(FILE* out, const VaddGpu& g) {
  std::fprintf(out, "GPU 0: %s %s bus=%s uuid=%s cus=%d visible=%d\n", g.product[0] ? g.product : VADD_FALLBACK_NAME, g.arch,
               g.bus, g.uuid, g.cus, g.visible);
}

inline void vadd_print_header(FILE* out, size_t n) { std::fprintf(out, "[Vector addition of %zu elements]\n", n); }

// `tail` goes before the closing brace: further members, each with its leading comma.
inline void vadd_print_json(FILE* out, size_t mismatches, size_t n, double kernel_ms, const VaddGpu& g, const char* tail = "") {
  std::fprintf(out, "{\"ok\":%s,\"n\":%zu,\"kernel_ms\":%.4f,\"uuid\":\"%s\",\"bus\":\"%s\",\"arch\":\"%s\",\"visible\":%d%s}\n",
               mismatches ? "false" : "true", n, kernel_ms, g.uuid, g.bus, g.arch, g.visible, tail);
}

// The last lines of a run, and the exit code that goes with them.
inline int vadd_print_verdict(FILE* out, size_t mismatches) {
  if (mismatches) {
    std::fprintf(out, "Result verification failed (%zu mismatches)\nTest FAILED\n", mismatches);
    return VADD_MISMATCHES;
  }
  std::fprintf(out, "Test PASSED\n");
  return VADD_PASSED;
}

}  // namespace amdkube
