// hsa-vector-add: the GPU-pod validation workload on the bare ROCr (HSA) runtime.
//
// Same contract as rocm-vector-add (kernels/vector_add.hip; the reference's cuda-vector-add test
// image, test/images/cuda-vector-add, run by test/e2e/scheduling/nvidia-gpus.go: success = exit 0
// and "Test PASSED"), same output lines (the visible GPU's product name, ISA, PCI bus id and
// UUID, so e2e tests can check the pod ran on exactly its assigned device), same input data and
// verification: all of that is kernels/vadd_contract.h, which both include. What it drops is the HIP
// runtime: a GPU pod's life is dominated by process
// start-up (docs/PERFORMANCE.md: ≈150 ms KFD release window + ≈50 ms ROCr init + ≈80 ms HIP init,
// work and exit), and everything the HIP layer adds on top of hsa_init — loading libamdhip64,
// device-property queries, the fat-binary registration, stream and blit-kernel set-up — is time
// the pod's GPU is held for nothing. Here the kernel (kernels/vadd_kernel.hip) is a bare gfx950
// code object embedded in this binary and loaded with the HSA code-object loader (kernels/hsa_min.h
// is the ROCr wrapper); the inputs are
// staged in host memory the GPU may access, and three AQL packets on one user-mode queue copy
// them into device memory, add, and copy the sum back (kernel copies: no SDMA engine to bring
// up, which alone cost ≈16 ms of the first version's life). On MI355X back-to-back pods of it
// live 250 ms (median of 15) against 320 ms for the HIP build (hack/exp/vadd_runtime_cmp.py,
// profiles/r3/hsa_vector_add.json). Skipping hsa_shut_down (--fast-exit) saves its ≈30 ms of
// user-space teardown but the next process then waits that much longer in the kernel's KFD
// release path, so the default shuts down cleanly.
//
// What is left of hsa_init after the wait in open("/dev/kfd") is file reading: ROCr reads about
// 8900 small files one by one (the CPU caches under /sys/devices/system/node, the KFD topology and
// /proc/cpuinfo, each walked twice; docs/PERFORMANCE.md "Prefetching hsa_init's file reads"). A
// helper thread started first thing in main reads them during that wait and this executable's
// fopen serves them to ROCr from memory (native/sysfs_prefetch.h): the part of hsa_init after the
// wait drops from 53 ms to 16 ms and a back-to-back pod from 280 ms to 240 ms (medians of 15 runs
// each; bench.py: 248 against 287 ms per step). The helper stops when the open returns, and a file
// it did not get to is read once by the thread that asks and kept for ROCr's second walk, so a
// pod with no predecessor, which has no wait to use, still gains (54 ms to 41 ms). --no-prefetch
// or AMDKUBE_VADD_PREFETCH=0 turn it off. AMDKUBE_VADD_TRACE=1 prints the phase times, hsa_init
// split at the /dev/kfd open, and its file I/O by path group (AMDKUBE_VADD_TRACE=paths: every
// path as well; native/io_trace.h).
//
//   hsa-vector-add [-n ELEMENTS] [--print-uuid] [--json] [--expect-devices K] [--fast-exit] [--no-prefetch]
#include <algorithm>
#include <cstddef>

#include "../native/io_trace.h"
#include "hsa_min.h"
#include "vadd_contract.h"

#ifndef VADD_CO_PATH
#error "VADD_CO_PATH must name the gfx950 code object to embed (native/build.py)"
#endif

extern "C" const unsigned char amdkube_vadd_co[];
extern "C" const unsigned char amdkube_vadd_co_end[];
__asm__(".section .rodata\n.balign 64\n.global amdkube_vadd_co\namdkube_vadd_co:\n.incbin \"" VADD_CO_PATH
        "\"\n.global amdkube_vadd_co_end\namdkube_vadd_co_end:\n.byte 0\n.previous\n");

namespace iotrace = amdkube::iotrace;
namespace prefetch = amdkube::prefetch;

// ROCr's and libdrm's calls find these before libc's: fopen serves the prefetched files, and all four
// feed the I/O trace. When the open of /dev/kfd returns, the wait the prefetch helper works in is
// over: from there on it would only compete with ROCr's own reads.
extern "C" FILE* fopen(const char* path, const char* mode) { return iotrace::traced_fopen(path, mode); }
extern "C" int fclose(FILE* f) { return iotrace::traced_fclose(f); }
extern "C" DIR* opendir(const char* path) { return iotrace::traced_opendir(path); }
extern "C" int open(const char* path, int flags, ...) {
  va_list ap;
  va_start(ap, flags);
  const int fd = iotrace::traced_open(path, flags, ap, prefetch::cancel);
  va_end(ap);
  return fd;
}

namespace {

using namespace amdkube;
using namespace amdkube::hsa;

struct CopyArgs {  // amdkube_copy: src, dst, float count, work-groups launched
  const float* src;
  float* dst;
  unsigned long long n;
  unsigned groups;
};

struct Args {  // amdkube_vadd: a, b, c, float count, work-groups launched
  const float* a;
  const float* b;
  float* c;
  unsigned long long n;
  unsigned groups;
};

struct Pod {   // what a run holds, in the order it is made
  hsa_agent_t gpu{};
  Program program;
  Kernel vadd, copy;
  size_t stride = 0;                          // floats from a to b to c: each starts on a 256-byte boundary
  float *ha = nullptr, *hb = nullptr, *hc = nullptr;   // host staging (GPU-accessible system memory), one allocation
  float *da = nullptr, *db = nullptr, *dc = nullptr;   // device buffers, one allocation
  hsa_signal_t done{};
  char* kargs = nullptr;                      // one kernarg block for the three packets
  size_t slot = 0;                            // each packet's share of it, 64-byte aligned
  uint32_t g_in = 0, g_add = 0;               // work-groups of the copy in, and of the add and the copy out
  hsa_queue_t* q = nullptr;
};

// hsa_init inside the trace window; with tracing on, where its time and its file I/O went
hsa_status_t init_runtime(iotrace::Phases& tr, bool prefetching) {
  const char* mode = std::getenv("AMDKUBE_VADD_TRACE");
  const int64_t init_begin = iotrace::window_begin(tr.on, mode && !std::strcmp(mode, "paths"));
  const hsa_status_t init = hsa_init();
  const int64_t init_end = iotrace::window_end();
  prefetch::cancel();   // nobody reads these files any more (hsa_init may have failed before its /dev/kfd open)
  if (init != HSA_STATUS_SUCCESS) return init;
  tr.mark("hsa_init");
  if (tr.on) {
    iotrace::report(stderr, init_begin, init_end);
    prefetch::join();
    const prefetch::Stats ps = prefetch::stats();
    std::fprintf(stderr, "[trace] prefetch %s files=%llu bytes=%llu helper_ms=%.3f hits=%llu misses=%llu distinct=%llu\n",
                 !prefetching ? "off" : (ps.dropped ? "dropped" : "on"), static_cast<unsigned long long>(ps.files),
                 static_cast<unsigned long long>(ps.bytes), ps.helper_ms, static_cast<unsigned long long>(ps.hits),
                 static_cast<unsigned long long>(ps.misses), static_cast<unsigned long long>(ps.distinct));
    tr.t = std::chrono::steady_clock::now();
  }
  return init;
}

// the embedded code object → executable → kernel descriptors
void load_kernels(Pod& p) {
  p.program = load_program(p.gpu, amdkube_vadd_co, amdkube_vadd_co_end - amdkube_vadd_co);
  p.vadd = kernel(p.program, p.gpu, "amdkube_vadd.kd");
  p.copy = kernel(p.program, p.gpu, "amdkube_copy.kd");
  if (p.vadd.kasz != offsetof(Args, groups) + sizeof(unsigned) || p.copy.kasz != offsetof(CopyArgs, groups) + sizeof(unsigned))
    throw Fail{"unexpected kernarg segment size", HSA_STATUS_ERROR};
}

void allocate_and_fill(Pod& p, const Pools& pools, size_t n) {
  p.stride = (n + 63) & ~static_cast<size_t>(63);   // the copy kernel moves 16-byte words
  const size_t span = 3 * p.stride * sizeof(float);
  check(hsa_amd_memory_pool_allocate(pools.host, span, 0, reinterpret_cast<void**>(&p.ha)), "host alloc");
  p.hb = p.ha + p.stride;
  p.hc = p.hb + p.stride;
  check(hsa_amd_memory_pool_allocate(pools.device, span, 0, reinterpret_cast<void**>(&p.da)), "device alloc");
  p.db = p.da + p.stride;
  p.dc = p.db + p.stride;
  check(hsa_amd_agents_allow_access(1, &p.gpu, nullptr, p.ha), "host access");
  vadd_fill_inputs(p.ha, p.hb, n);
  std::memset(p.hc, 0xff, n * sizeof(float));   // NaN: an element no kernel wrote counts as a mismatch
}

// the completion signal, the three packets' arguments and the queue
void prepare_queue(Pod& p, const Pools& pools, size_t n, int cus) {
  check(hsa_signal_create(1, 0, nullptr, &p.done), "signal");
  p.slot = 64 * ((std::max<uint32_t>(p.vadd.kasz, p.copy.kasz) + 63) / 64);
  check(hsa_amd_memory_pool_allocate(pools.kernarg, 3 * p.slot, 0, reinterpret_cast<void**>(&p.kargs)), "kernarg alloc");
  check(hsa_amd_agents_allow_access(1, &p.gpu, nullptr, p.kargs), "kernarg access");
  std::memset(p.kargs, 0, 3 * p.slot);
  // one work-group per 256 whole 16-byte words
  p.g_in = stream_grid(2 * p.stride / 4, cus, VADD_BLOCKS_PER_CU);
  p.g_add = stream_grid(n / 4, cus, VADD_BLOCKS_PER_CU);
  *reinterpret_cast<CopyArgs*>(p.kargs) = CopyArgs{p.ha, p.da, 2 * static_cast<unsigned long long>(p.stride), p.g_in};
  *reinterpret_cast<Args*>(p.kargs + p.slot) = Args{p.da, p.db, p.dc, static_cast<unsigned long long>(n), p.g_add};
  *reinterpret_cast<CopyArgs*>(p.kargs + 2 * p.slot) = CopyArgs{p.dc, p.hc, static_cast<unsigned long long>(n), p.g_add};
  check(hsa_queue_create(p.gpu, 64, HSA_QUEUE_TYPE_SINGLE, nullptr, nullptr, UINT32_MAX, UINT32_MAX, &p.q), "queue");
}

// the three packets, in order on the one queue; returns the time from the first doorbell to the last completion
double submit_and_wait(Pod& p) {
  const auto t0 = std::chrono::steady_clock::now();
  dispatch(p.q, p.copy, p.kargs, p.g_in, VADD_WG, hsa_signal_t{0});                 // host a,b → device
  dispatch(p.q, p.vadd, p.kargs + p.slot, p.g_add, VADD_WG, hsa_signal_t{0});       // c = a + b on device memory
  dispatch(p.q, p.copy, p.kargs + 2 * p.slot, p.g_add, VADD_WG, p.done);            // device c → host
  wait_zero(p.done, "vector add");
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// In this order. --fast-exit skips it, and an error leaves without it.
void teardown(Pod& p) {
  hsa_queue_destroy(p.q);
  hsa_signal_destroy(p.done);
  hsa_amd_memory_pool_free(p.kargs);
  hsa_amd_memory_pool_free(p.da);
  hsa_amd_memory_pool_free(p.ha);
  hsa_executable_destroy(p.program.exe);
  hsa_code_object_reader_destroy(p.program.reader);
  hsa_shut_down();
}

int run(const VaddOptions& o, bool prefetching) {
  if (o.n == 0) {
    std::fprintf(stderr, "hsa-vector-add: -n must be > 0\n");
    return VADD_ERROR;
  }
  iotrace::Phases tr{std::getenv("AMDKUBE_VADD_TRACE") != nullptr};
  try {
    // no /dev/kfd (or no render node) for this container: ROCr cannot open a GPU at all
    if (const hsa_status_t init = init_runtime(tr, prefetching); init != HSA_STATUS_SUCCESS)
      return vadd_print_no_gpu(stderr, (std::string("hsa_init: ") + status_text(init)).c_str());

    Agents ag;
    check(hsa_iterate_agents(on_agent, &ag), "iterate agents");
    const int count = static_cast<int>(ag.gpus.size());
    if (const int rc = vadd_check_device_count(stderr, count, o.expect_devices); rc >= 0) return rc;
    if (!ag.have_cpu) throw Fail{"no CPU agent", HSA_STATUS_ERROR};
    Pod p;
    p.gpu = ag.gpus[0];
    const GpuId id = identify(p.gpu);
    const VaddGpu gpu{id.product.c_str(), id.arch.c_str(), id.bus.c_str(), id.uuid.c_str(), static_cast<int>(id.cus), count};
    if (o.print_uuid || !o.json) vadd_print_identity(stdout, gpu);
    vadd_print_header(stdout, o.n);
    tr.mark("agents");

    const Pools pools = find_pools(p.gpu, ag.cpu);
    load_kernels(p);
    tr.mark("code object");

    allocate_and_fill(p, pools, o.n);
    tr.mark("alloc + fill");

    prepare_queue(p, pools, o.n, gpu.cus);
    tr.mark("queue");

    const double kernel_ms = submit_and_wait(p);
    tr.mark("gpu work");

    const size_t bad = vadd_count_mismatches(p.ha, p.hb, p.hc, o.n);
    tr.mark("verify");

    if (!o.fast_exit) {
      teardown(p);
      tr.mark("shut down");
    }
    if (o.json)
      vadd_print_json(stdout, bad, o.n, kernel_ms, gpu,
                      prefetching ? ",\"runtime\":\"hsa\",\"prefetch\":true" : ",\"runtime\":\"hsa\",\"prefetch\":false");
    return vadd_print_verdict(stdout, bad);
  } catch (const Fail& f) {
    std::fprintf(stderr, "hsa-vector-add: %s: %s\n", f.what.c_str(), status_text(f.st));
    return VADD_ERROR;
  }
}

}  // namespace

int main(int argc, char** argv) {
  // first thing, before hsa_init: the helper reads what hsa_init will read while it waits in open("/dev/kfd")
  const amdkube::VaddOptions o = amdkube::vadd_parse_args(argc, argv);   // opens nothing, calls nothing in ROCr
  const bool prefetching = prefetch::enabled_by_env() && !o.no_prefetch;
  if (prefetching) prefetch::start();
  const int rc = run(o, prefetching);
  prefetch::join();   // on every path out of run(), the error returns included
  return rc;
}
