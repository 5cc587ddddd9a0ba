// amdkube GPU validation workloads for MI355X (gfx950 / CDNA4).
//
// The reference's only GPU workload is the CUDA-samples vectorAdd image its e2e tests run
// in GPU pods (test/images/cuda-vector-add/Dockerfile:15-26; 50,000 fp32 elements), plus
// device health that comes solely from the plugin (api.proto:97). amdkube replaces that
// with five CDNA4-native workloads behind the standalone pod binaries (rocm-vector-add,
// hbm-probe, gpu-burn, mfma-check, cu-check) and the in-process Python extension (_hipops).
// This header is the base: the first three, and mix32 and the vector types the checks build on.
//
//   vector add   wave64 grid-stride, 16-B (float4) loads, grid sized to the chip
//   HBM probe    address-hashed write / verify / read / copy over buffers larger than
//                the 256 MiB Infinity Cache, 16 B per lane, 4-deep unrolled so every CU
//                keeps ~32 KiB in flight — the pattern MI355X_MICROARCH measures at
//                ~6.3 TB/s; verify counts mismatches (ECC-sensitive health check)
//   MFMA burn    register-resident v_mfma_f32_32x32x16_bf16 chains, 2 independent
//                accumulators per wave, for matrix-core load / utilisation validation
//
// The checks are headers of their own, each including this one; a program includes what it launches:
//   MFMA check   (mfma_check.h) LDS-staged 64x64 bf16 tiles whose every result is compared:
//                round 0 with exact int32 arithmetic, later rounds bitwise with round 0;
//                (mfma_check_lp.h) the same on the FP8 MFMA and the block-scaled MXFP8 / MXFP4 forms
//   CU check     (cu_check.h) one workgroup per CU with all 160 KiB of LDS: a march over the LDS, the
//                same multiply-adds on the fp32, packed-fp32, fp64 and integer pipes, the
//                transcendental unit on two waves, and the XCD / shader engine / CU it ran on
//   HBM check    (hbm_check.h, behind hbm-check) a MATS++ march on the pattern below over a region planned by
//                hbm_plan.h: every bit read in both states, every error with its offset, bits and place
// The host side is shared: gpu_host.h (AK_HIP, DevInfo, DevBuf, GpuTimer), check_core.h (calibration,
// self-test flip positions, list splitting) and vadd_contract.h (the pod workload's contract, which
// hsa-vector-add shares: flags, inputs, verification, stream_grid, output lines, exit codes); the last
// two are plain C++, self-tested on the CPU.
//
// Every launch is bounded by construction (grid-stride loops over checked sizes) and uses
// no inter-workgroup synchronisation, so no launch can hang the device.
#pragma once

#include "check_core.h"
#include "gpu_host.h"
#include "vadd_contract.h"

namespace amdkube {

// ---------------------------------------------------------------------------- kernels
// Each workgroup owns one contiguous chunk of the float4 range (streaming, non-temporal): on
// MI355X the chunked layout at 64 WG/CU moves 5.95 TB/s of a+b->c traffic against 5.46 TB/s for
// the grid-stride loop (hack/exp/write_sweep.hip, 3 x 1 GiB): VADD_BLOCKS_PER_CU (vadd_contract.h).
typedef float v4f __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(VADD_WG) void vadd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ c, size_t n) {
  const size_t n4 = n >> 2;
  const v4f* a4 = reinterpret_cast<const v4f*>(a);
  const v4f* b4 = reinterpret_cast<const v4f*>(b);
  v4f* c4 = reinterpret_cast<v4f*>(c);
  const size_t per = (n4 + gridDim.x - 1) / gridDim.x;
  const size_t lo = static_cast<size_t>(blockIdx.x) * per;
  const size_t hi = lo + per < n4 ? lo + per : n4;
  for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
    __builtin_nontemporal_store(__builtin_nontemporal_load(a4 + i) + __builtin_nontemporal_load(b4 + i), c4 + i);
  if (blockIdx.x == 0)                               // the < 4 trailing scalars
    for (size_t i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) c[i] = a[i] + b[i];
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the checks' hash of (seed, workgroup, index)
__device__ __forceinline__ uint32_t mix32(uint32_t seed, uint32_t block, uint32_t index) {
  return mix32(mix32(seed ^ (0x9e3779b9u * (block + 1))) + index);
}

// Where a wave runs: the raw HW_ID and XCC_ID words (the field layout and what an MI355X shows in them:
// cu_check.h) and their decoding into (xcc, se, sh, cu). For the checks that say where an error was seen.
// s_getreg_b32 operand: register id, offset 0, all 32 bits
constexpr int CU_HWREG_HW_ID = 4 | (31 << 11);
constexpr int CU_HWREG_XCC_ID = 20 | (31 << 11);

struct CuLocation {
  int xcc = 0, se = 0, sh = 0, cu = 0;
  uint32_t key() const { return static_cast<uint32_t>(xcc) << 12 | se << 8 | sh << 4 | cu; }
};

inline CuLocation cu_decode_location(uint32_t hw_id, uint32_t xcc_id) {
  CuLocation l;
  l.xcc = xcc_id & 15u;
  l.cu = (hw_id >> 8) & 15u;
  l.sh = (hw_id >> 12) & 1u;
  l.se = (hw_id >> 13) & 7u;
  return l;
}

__device__ __forceinline__ uint4 pattern(size_t i, uint32_t seed) {
  uint32_t base = static_cast<uint32_t>(i * 4) ^ seed ^ static_cast<uint32_t>(i >> 30);
  return make_uint4(mix32(base), mix32(base + 1), mix32(base + 2), mix32(base + 3));
}

// Streaming kernels: 8 independent 16-B loads in flight per lane, non-temporal (streaming) loads
// and stores so a 4 GiB sweep does not thrash the per-XCD L2 / MALL, and a grid of 32 blocks/CU
// (tuned on MI355X by hack/exp/hbm_variants.hip: copy 4.90 -> 5.29 TB/s, read 5.52 -> 6.77 TB/s).
constexpr int HBM_UNROLL = 8;
constexpr int HBM_BLOCKS_PER_CU = 32;
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4u ld_nt(const v4u* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st_nt(v4u* p, v4u v) { __builtin_nontemporal_store(v, p); }

// Pure writes go out with the default cache policy as a narrow grid-stride "front": half as many
// workgroups as CUs (128 on MI355X), 256 lanes, two 16-B stores in flight per lane, so the whole
// chip writes one ~1 MiB window that sweeps the buffer in address order and the HBM sees long
// runs of consecutive pages. Round-4 sweeps on MI355X, hashed pattern, 1 / 4 GiB
// (hack/exp/write_sweep4.hip, front_sweep5.hip): front 128 x 2-deep 6.82-6.96 / 6.83-7.09 TB/s,
// front 96 5.3, front 160 6.1, front 256 5.8-6.0, per-workgroup chunks at 16 WG/CU 5.85 / 5.7,
// hipMemsetD32 (the runtime's own 256 x 256 front) 6.45-6.75. Copies keep nt on both sides and
// run chunked at 128 WG/CU (5.72 / 5.80 TB/s on 1 / 4 GiB); fronts did not help them
// (copy_sweep4.hip: 5.1-5.9).
constexpr int HBM_WRITE_UNROLL = 2;
inline int write_front_grid(int cu_count) { return cu_count > 1 ? cu_count / 2 : 1; }
__device__ __forceinline__ void st_plain(v4u* p, v4u v) { *p = v; }

__device__ __forceinline__ v4u pattern_v(size_t i, uint32_t seed) {
  uint4 p = pattern(i, seed);
  return v4u{p.x, p.y, p.z, p.w};
}

// Per-workgroup contiguous chunks (see the copy kernel below): the round-3 sweep on MI355X gives
// the hashed-pattern write 5.41 TB/s chunked against 4.63 grid-strided (hack/exp/write_sweep.hip).
__device__ __forceinline__ void chunk_of(size_t n16, size_t* lo, size_t* hi) {
  const size_t per = (n16 + gridDim.x - 1) / gridDim.x;
  *lo = static_cast<size_t>(blockIdx.x) * per;
  *hi = *lo + per < n16 ? *lo + per : n16;
}

__global__ __launch_bounds__(256) void hbm_write_kernel(v4u* __restrict__ buf, size_t n16, uint32_t seed) {
  const size_t st = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (; i + (HBM_WRITE_UNROLL - 1) * st < n16; i += HBM_WRITE_UNROLL * st) {
#pragma unroll
    for (int u = 0; u < HBM_WRITE_UNROLL; ++u) st_plain(buf + i + u * st, pattern_v(i + u * st, seed));
  }
  for (; i < n16; i += st) st_plain(buf + i, pattern_v(i, seed));
}

__device__ __forceinline__ unsigned mismatches(v4u v, v4u e) {
  return (v.x != e.x) + (v.y != e.y) + (v.z != e.z) + (v.w != e.w);
}

__global__ __launch_bounds__(256) void hbm_verify_kernel(const v4u* __restrict__ buf, size_t n16, uint32_t seed,
                                                         unsigned long long* __restrict__ errors) {
  size_t lo, hi;
  chunk_of(n16, &lo, &hi);
  const size_t b = blockDim.x;
  unsigned long long bad = 0;
  size_t i = lo + threadIdx.x;
  for (; i + (HBM_UNROLL - 1) * b < hi; i += HBM_UNROLL * b) {
    v4u v[HBM_UNROLL];
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) v[u] = ld_nt(buf + i + u * b);
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) bad += mismatches(v[u], pattern_v(i + u * b, seed));
  }
  for (; i < hi; i += b) bad += mismatches(ld_nt(buf + i), pattern_v(i, seed));
  if (bad) atomicAdd(errors, bad);  // errors are rare: no contention on a healthy part
}

__global__ __launch_bounds__(256) void hbm_read_kernel(const v4u* __restrict__ buf, size_t n16, uint32_t* sink) {
  size_t lo, hi;
  chunk_of(n16, &lo, &hi);
  const size_t b = blockDim.x;
  uint32_t acc = 0;
  size_t i = lo + threadIdx.x;
  for (; i + (HBM_UNROLL - 1) * b < hi; i += HBM_UNROLL * b) {
    v4u v[HBM_UNROLL];
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) v[u] = ld_nt(buf + i + u * b);
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
  }
  for (; i < hi; i += b) {
    v4u v = ld_nt(buf + i);
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x9e3779b9u) sink[0] = acc;  // keeps the loads live
}

// Copy: each workgroup owns one contiguous chunk and walks it in 8 x 256-lane tiles (8 x 16 B
// in flight per lane), so every XCD streams long runs of consecutive DRAM pages instead of the
// grid-stride interleave; 64 workgroups/CU. Round-3 sweep on MI355X (hack/exp/copy_sweep.hip,
// 2 x 4 GiB): grid-stride 32/CU 5.01 TB/s, grid-stride 64/CU 5.20, chunked 64/CU 5.53,
// hipMemcpyDtoD 4.70.
constexpr int HBM_COPY_BLOCKS_PER_CU = 128;

__global__ __launch_bounds__(256) void hbm_copy_kernel(const v4u* __restrict__ src, v4u* __restrict__ dst,
                                                       size_t n16) {
  const size_t per = (n16 + gridDim.x - 1) / gridDim.x;
  const size_t lo = static_cast<size_t>(blockIdx.x) * per;
  const size_t hi = lo + per < n16 ? lo + per : n16;
  size_t i = lo + threadIdx.x;
  for (; i + (HBM_UNROLL - 1) * blockDim.x < hi; i += static_cast<size_t>(HBM_UNROLL) * blockDim.x) {
    v4u v[HBM_UNROLL];
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) v[u] = ld_nt(src + i + u * blockDim.x);
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) st_nt(dst + i + u * blockDim.x, v[u]);
  }
  for (; i < hi; i += blockDim.x) st_nt(dst + i, ld_nt(src + i));
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 2 independent 32x32x16 bf16 MFMA accumulator chains per wave, operands in registers.
__global__ __launch_bounds__(256) void mfma_burn_kernel(float* __restrict__ out, int iters) {
  bf16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = static_cast<__bf16>(1.0f / (1 + ((threadIdx.x + j) & 7)));
    b[j] = static_cast<__bf16>(0.001f * (j + 1));
  }
  f32x16 c0 = {}, c1 = {};
  for (int it = 0; it < iters; ++it) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, c1, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += c0[j] + c1[j];
  out[static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x] = s;
}

// One wave computes C[32x32] = A[32xK] * B[Kx32] (bf16 in, fp32 out) with the burn's MFMA,
// v_mfma_f32_32x32x16_bf16, K/16 chained steps. Operand lane maps (CDNA4): lane l, r = l&31,
// h = l>>5 holds A[r][8h+j] and B[8h+j][r] (j = 0..7); accumulator register q of lane l is
// C[(q&3) + 8(q>>2) + 4h][r]. The numerics check of the matrix-core path: the same layout the
// burn relies on, against a torch fp32 matmul (tests/test_gpu.py).
__global__ __launch_bounds__(64) void mfma_tile_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                       float* __restrict__ C, int k_steps) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  const int K = 16 * k_steps;
  f32x16 acc = {};
  for (int ks = 0; ks < k_steps; ++ks) {
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = A[r * K + ks * 16 + 8 * h + j];
      b[j] = B[(ks * 16 + 8 * h + j) * 32 + r];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) C[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
}

// ---------------------------------------------------------------------------- runners
// (stream_grid, the pod workload's inputs and its verification: vadd_contract.h)
struct VaddResult {
  bool ok = false;
  double kernel_ms = 0;
  size_t mismatches = 0;
};

inline VaddResult run_vector_add(size_t n, int dev) {
  VaddResult r;
  if (n == 0) throw std::invalid_argument("n must be > 0");
  AK_HIP(hipSetDevice(dev));
  DevInfo info = dev_info(dev);
  std::vector<float> ha(n), hb(n);
  vadd_fill_inputs(ha.data(), hb.data(), n);
  DevBuf da(ha), db(hb), dc(n * sizeof(float));
  dc.fill(0xff);   // NaN, as hsa-vector-add fills its c: an element the kernel never wrote is a mismatch
  GpuTimer timer;
  const int grid = stream_grid((n + 3) / 4, info.cu_count, VADD_BLOCKS_PER_CU);
  r.kernel_ms = timer.time([&] {
    hipLaunchKernelGGL(vadd_kernel, dim3(grid), dim3(VADD_WG), 0, 0, da.as<float>(), db.as<float>(), dc.as<float>(), n);
    AK_HIP(hipGetLastError());
  });
  const std::vector<float> hc = dc.download<float>();
  r.mismatches = vadd_count_mismatches(ha.data(), hb.data(), hc.data(), n);
  r.ok = r.mismatches == 0;
  return r;
}

// ---- host-supplied data: the kernels on caller-provided inputs (bitwise against numpy / torch on the CPU)
// `grid` is the number of workgroups to launch; 0 takes the production grid, which comes from the CU count
// and reaches its cap only at tens of MiB. A test passes its own to get, at a few KiB, chunks that are
// empty, ragged, or long enough for the unrolled loops (tests/test_gpu_stream_kernels.py). Every kernel
// here is right at any grid: it derives its chunks or its stride from gridDim.
constexpr int HOST_GRID_MAX = 65536;

inline int host_grid(int grid, int production) {
  if (grid < 0 || grid > HOST_GRID_MAX) throw std::invalid_argument("grid must be in [0, 65536] (0: the production grid)");
  return grid ? grid : production;
}

// Outputs start as 0xff bytes (NaN as fp32), so an element the kernel skipped cannot pass on what the
// allocation happened to hold.
// c = a + b on the device with the pod workload's vadd_kernel
inline std::vector<float> vector_add_host(const std::vector<float>& a, const std::vector<float>& b, int dev, int grid = 0) {
  if (a.size() != b.size()) throw std::invalid_argument("a and b differ in length");
  AK_HIP(hipSetDevice(dev));
  const size_t n = a.size();
  grid = host_grid(grid, stream_grid((n + 3) / 4, dev_info(dev).cu_count, VADD_BLOCKS_PER_CU));
  DevBuf da(a), db(b), dc(n * sizeof(float));
  dc.fill(0xff);
  hipLaunchKernelGGL(vadd_kernel, dim3(grid), dim3(VADD_WG), 0, 0, da.as<const float>(), db.as<const float>(), dc.as<float>(), n);
  AK_HIP(hipGetLastError());
  return dc.download<float>();
}

// the HBM probe's write pattern for n16 16-byte words (checked against a numpy re-derivation)
inline std::vector<uint32_t> hbm_pattern_host(size_t n16, uint32_t seed, int dev, int grid = 0) {
  AK_HIP(hipSetDevice(dev));
  grid = host_grid(grid, write_front_grid(dev_info(dev).cu_count));
  DevBuf d(n16 * 16);
  d.fill(0xff);
  hipLaunchKernelGGL(hbm_write_kernel, dim3(grid), dim3(256), 0, 0, d.as<v4u>(), n16, seed);
  AK_HIP(hipGetLastError());
  return d.download<uint32_t>();
}

// the probe's verify kernel on caller data: mismatching 32-bit words against the pattern
inline unsigned long long hbm_verify_host(const std::vector<uint32_t>& words, uint32_t seed, int dev, int grid = 0) {
  if (words.size() % 4) throw std::invalid_argument("need a whole number of 16-byte words");
  AK_HIP(hipSetDevice(dev));
  const size_t n16 = words.size() / 4;
  grid = host_grid(grid, stream_grid(n16, dev_info(dev).cu_count, HBM_BLOCKS_PER_CU));
  DevBuf d(words), e(sizeof(unsigned long long), DevBuf::zeroed);
  hipLaunchKernelGGL(hbm_verify_kernel, dim3(grid), dim3(256), 0, 0, d.as<const v4u>(), n16, seed, e.as<unsigned long long>());
  AK_HIP(hipGetLastError());
  return e.download<unsigned long long>()[0];
}

// the probe's read kernel on caller data: the XOR of every 32-bit word it loaded, if that is the one value
// the kernel stores (0x9e3779b9), else 0. A buffer of zeros with that word in one place says whether the
// place was read.
inline uint32_t hbm_read_host(const std::vector<uint32_t>& words, int grid, int dev) {
  if (words.size() % 4) throw std::invalid_argument("need a whole number of 16-byte words");
  AK_HIP(hipSetDevice(dev));
  const size_t n16 = words.size() / 4;
  grid = host_grid(grid, stream_grid(n16, dev_info(dev).cu_count, HBM_BLOCKS_PER_CU));
  DevBuf d(words), sink(sizeof(uint32_t), DevBuf::zeroed);
  hipLaunchKernelGGL(hbm_read_kernel, dim3(grid), dim3(256), 0, 0, d.as<const v4u>(), n16, sink.as<uint32_t>());
  AK_HIP(hipGetLastError());
  return sink.download<uint32_t>()[0];
}

// the probe's copy kernel on caller data
inline std::vector<uint32_t> hbm_copy_host(const std::vector<uint32_t>& words, int dev, int grid = 0) {
  if (words.size() % 4) throw std::invalid_argument("need a whole number of 16-byte words");
  AK_HIP(hipSetDevice(dev));
  const size_t n16 = words.size() / 4;
  grid = host_grid(grid, stream_grid(n16, dev_info(dev).cu_count, HBM_COPY_BLOCKS_PER_CU));
  DevBuf s(words), d(n16 * 16);
  d.fill(0xff);
  hipLaunchKernelGGL(hbm_copy_kernel, dim3(grid), dim3(256), 0, 0, s.as<const v4u>(), d.as<v4u>(), n16);
  AK_HIP(hipGetLastError());
  return d.download<uint32_t>();
}

// ---- hsa-vector-add's kernels in this process: the bare code object that program embeds (vadd_kernel.hip,
// built by native/build.py), loaded from its file and launched through HIP's module API with the packed
// kernarg blocks of hsa_vector_add.cpp. `groups` is both the grid and the kernels' last argument.
struct GpuModule {
  hipModule_t m = nullptr;
  explicit GpuModule(const std::string& path) {
    hipError_t e = hipModuleLoad(&m, path.c_str());
    if (e != hipSuccess) throw std::runtime_error("hipModuleLoad(" + path + "): " + hipGetErrorString(e));
  }
  ~GpuModule() { (void)hipModuleUnload(m); }
  GpuModule(const GpuModule&) = delete;
  GpuModule& operator=(const GpuModule&) = delete;
  hipFunction_t function(const char* name) const {
    hipFunction_t f = nullptr;
    AK_HIP(hipModuleGetFunction(&f, m, name));
    return f;
  }
  // one launch of groups x VADD_WG on the null stream with `size` bytes of kernel arguments
  void launch(hipFunction_t f, unsigned groups, void* args, size_t size) const {
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    AK_HIP(hipModuleLaunchKernel(f, groups, 1, 1, VADD_WG, 1, 1, 0, nullptr, nullptr, config));
  }
};

struct __attribute__((packed)) CoVaddArgs {   // amdkube_vadd's kernarg segment: hsa_vector_add.cpp, Args
  const float *a, *b;
  float* c;
  unsigned long long n;
  unsigned groups;
};
struct __attribute__((packed)) CoCopyArgs {   // amdkube_copy's: hsa_vector_add.cpp, CopyArgs
  const float* src;
  float* dst;
  unsigned long long n;
  unsigned groups;
};
static_assert(sizeof(CoVaddArgs) == 36 && sizeof(CoCopyArgs) == 28, "the kernarg segment sizes hsa-vector-add checks");

inline unsigned co_groups(int groups) {
  if (groups < 1 || groups > HOST_GRID_MAX) throw std::invalid_argument("groups must be in [1, 65536]");
  return static_cast<unsigned>(groups);
}

// c = a + b with amdkube_vadd of the code object at `path`
inline std::vector<float> co_vadd_host(const std::string& path, const std::vector<float>& a, const std::vector<float>& b,
                                       int groups, int dev) {
  if (a.size() != b.size()) throw std::invalid_argument("a and b differ in length");
  const unsigned g = co_groups(groups);
  AK_HIP(hipSetDevice(dev));
  DevBuf da(a), db(b), dc(a.size() * sizeof(float));
  dc.fill(0xff);
  GpuModule mod(path);   // unloaded on every way out, before the buffers go; the download waits for the kernel
  CoVaddArgs args{da.as<const float>(), db.as<const float>(), dc.as<float>(), a.size(), g};
  mod.launch(mod.function("amdkube_vadd"), g, &args, sizeof args);
  return dc.download<float>();
}

// a copy of src made by amdkube_copy of the code object at `path`
inline std::vector<float> co_copy_host(const std::string& path, const std::vector<float>& src, int groups, int dev) {
  const unsigned g = co_groups(groups);
  AK_HIP(hipSetDevice(dev));
  DevBuf ds(src), dd(src.size() * sizeof(float));
  dd.fill(0xff);
  GpuModule mod(path);
  CoCopyArgs args{ds.as<const float>(), dd.as<float>(), src.size(), g};
  mod.launch(mod.function("amdkube_copy"), g, &args, sizeof args);
  return dd.download<float>();
}

// C[32x32] fp32 = A[32xK] bf16 * B[Kx32] bf16 on one wave (K a multiple of 16, <= 1024)
inline std::vector<float> mfma_tile_host(const std::vector<uint16_t>& a_bits, const std::vector<uint16_t>& b_bits,
                                         int k, int dev) {
  if (k <= 0 || k % 16 || k > 1024) throw std::invalid_argument("K must be a positive multiple of 16, at most 1024");
  if (a_bits.size() != static_cast<size_t>(32 * k) || b_bits.size() != static_cast<size_t>(32 * k))
    throw std::invalid_argument("A must be 32xK and B Kx32 bf16");
  AK_HIP(hipSetDevice(dev));
  DevBuf da(a_bits), db(b_bits), dc(32 * 32 * sizeof(float));
  hipLaunchKernelGGL(mfma_tile_kernel, dim3(1), dim3(64), 0, 0, da.as<const __bf16>(), db.as<const __bf16>(), dc.as<float>(),
                     k / 16);
  AK_HIP(hipGetLastError());
  return dc.download<float>();
}

struct HbmResult {
  double write_gbps = 0, read_gbps = 0, copy_gbps = 0, verify_gbps = 0;
  unsigned long long errors = 0;
  size_t bytes = 0;
  int iters = 0;
};

inline HbmResult run_hbm_probe(size_t bytes, int iters, int dev, uint32_t seed = 0x5eedu) {
  HbmResult r;
  if (iters < 1) iters = 1;
  bytes &= ~static_cast<size_t>(15);
  if (bytes < (1u << 20)) throw std::invalid_argument("hbm probe needs at least 1 MiB");
  AK_HIP(hipSetDevice(dev));
  DevInfo info = dev_info(dev);
  const size_t n16 = bytes / 16;
  DevBuf da(bytes), db(bytes), derrs(sizeof(unsigned long long), DevBuf::zeroed), dsink(sizeof(uint32_t));
  v4u *a = da.as<v4u>(), *b = db.as<v4u>();
  unsigned long long* errs = derrs.as<unsigned long long>();
  uint32_t* sink = dsink.as<uint32_t>();
  GpuTimer timer;
  const int grid = stream_grid(n16, info.cu_count, HBM_BLOCKS_PER_CU);
  auto timed = [&](auto&& launch) {
    for (int w = 0; w < 3; ++w) launch();  // warm-up: page-in / first touch, and the clock ramp
    AK_HIP(hipGetLastError());
    return timer.time([&] {
      for (int it = 0; it < iters; ++it) launch();
    }) / iters;
  };
  const int write_grid = write_front_grid(info.cu_count);
  double w = timed([&] { hipLaunchKernelGGL(hbm_write_kernel, dim3(write_grid), dim3(256), 0, 0, a, n16, seed); });
  double rd = timed([&] { hipLaunchKernelGGL(hbm_read_kernel, dim3(grid), dim3(256), 0, 0, a, n16, sink); });
  const int copy_grid = stream_grid(n16, info.cu_count, HBM_COPY_BLOCKS_PER_CU);
  double cp = timed([&] { hipLaunchKernelGGL(hbm_copy_kernel, dim3(copy_grid), dim3(256), 0, 0, a, b, n16); });
  derrs.zero();
  const double vms = timer.time([&] {
    hipLaunchKernelGGL(hbm_verify_kernel, dim3(grid), dim3(256), 0, 0, b, n16, seed, errs);
    AK_HIP(hipGetLastError());
  });
  r.errors = derrs.download<unsigned long long>()[0];
  r.bytes = bytes;
  r.iters = iters;
  r.write_gbps = bytes / (w * 1e6);
  r.read_gbps = bytes / (rd * 1e6);
  r.copy_gbps = 2.0 * bytes / (cp * 1e6);
  r.verify_gbps = bytes / (vms * 1e6);
  return r;
}

struct BurnResult {
  double ms = 0, tflops = 0;
  long long iters = 0;
  int blocks = 0;
};

inline BurnResult run_mfma_burn(double target_ms, int dev) {
  BurnResult r;
  AK_HIP(hipSetDevice(dev));
  DevInfo info = dev_info(dev);
  const int blocks = (info.cu_count > 0 ? info.cu_count : 256) * 4;  // 16 waves / CU
  DevBuf out(static_cast<size_t>(blocks) * 256 * sizeof(float));
  GpuTimer timer;
  const Calibrated c = calibrate(
      [&](int iters, int) {
        return timer.time([&] {
          hipLaunchKernelGGL(mfma_burn_kernel, dim3(blocks), dim3(256), 0, 0, out.as<float>(), iters);
          AK_HIP(hipGetLastError());
        });
      },
      2000, 200000000, 0, target_ms, 0);
  const double flops = static_cast<double>(blocks) * 4 /*waves*/ * c.rounds * 2 /*chains*/ * (2.0 * 32 * 32 * 16);
  r.ms = c.ms;
  r.iters = c.rounds;
  r.blocks = blocks;
  r.tflops = flops / (c.ms * 1e9);
  return r;
}

}  // namespace amdkube
