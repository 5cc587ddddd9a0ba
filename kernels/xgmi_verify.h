// The verifier of xgmi-probe's all-reduce (kernels/xgmi_probe.cpp) and its reach from _hipops: a kernel
// that fills a rank's contribution, one that counts the elements of a result that differ from the expected
// sum and keeps the first of them, and the self-test's flip. The arithmetic and the bound that makes the
// comparison exact are in xgmi_pattern.h. Every loop is a grid-stride loop over a checked count, right at
// any grid, and there is no inter-workgroup synchronisation.
#pragma once

#include "gpu_common.h"
#include "xgmi_pattern.h"

namespace amdkube {

constexpr int XGMI_GRID = 1024;          // workgroups of a production launch: one pass over at most 64 MiB
constexpr int XGMI_WG = 256;
constexpr int XGMI_RECORDS = 16;
constexpr int XGMI_MAX_FLIPS = 64;

// got and want are the raw fp32 bits
struct XgmiRecord {
  unsigned long long index;
  uint32_t got, want;
};

struct XgmiCount {
  unsigned long long wrong = 0;
  std::vector<XgmiRecord> records;       // the first XGMI_RECORDS at most, in no particular order
};

__global__ __launch_bounds__(XGMI_WG) void xgmi_fill_kernel(float* __restrict__ buf, size_t count, int rank, uint32_t seed) {
  for (size_t e = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; e < count;
       e += static_cast<size_t>(gridDim.x) * blockDim.x)
    buf[e] = xgmi_value(seed, rank, e);
}

// A NaN differs from everything, so an element that is one counts as wrong.
__global__ __launch_bounds__(XGMI_WG) void xgmi_count_kernel(const float* __restrict__ buf, size_t count, int n, uint32_t seed,
                                                             unsigned long long* __restrict__ wrong,
                                                             unsigned* __restrict__ nrec, XgmiRecord* __restrict__ recs) {
  unsigned long long bad = 0;
  unsigned mine = 0;
  for (size_t e = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; e < count;
       e += static_cast<size_t>(gridDim.x) * blockDim.x) {
    const float got = buf[e], want = xgmi_want(seed, n, e);
    if (got != want) {
      ++bad;
      if (mine < XGMI_RECORDS) {  // a lane asks for at most 16 slots however long it runs
        ++mine;
        const unsigned slot = atomicAdd(nrec, 1u);
        if (slot < XGMI_RECORDS) recs[slot] = XgmiRecord{e, __float_as_uint(got), __float_as_uint(want)};
      }
    }
  }
  if (bad) atomicAdd(wrong, bad);  // one per lane that saw a mismatch: none on a healthy fabric
}

// the self-test: the low mantissa bit of element pos[f], for f < n, with an ordinary load and store
__global__ __launch_bounds__(64) void xgmi_flip_kernel(float* __restrict__ buf, size_t count, const uint32_t* __restrict__ pos,
                                                       int n) {
  const int f = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= n || f >= XGMI_MAX_FLIPS) return;
  const uint32_t p = pos[f];
  if (p >= count) return;
  reinterpret_cast<uint32_t*>(buf)[p] ^= 1u;
}

// ---------------------------------------------------------------------------- runners
inline void xgmi_check_ranks(int ranks) {
  if (ranks < 1 || ranks > XGMI_MAX_RANKS) throw std::invalid_argument("ranks must be in [1, 64]");
}

// The three below work on memory of the current device and queue on `stream`; `grid` is a number of workgroups.
inline void xgmi_fill_device(float* buf, size_t count, int rank, uint32_t seed, int grid, hipStream_t stream) {
  if (rank < 0 || rank >= XGMI_MAX_RANKS) throw std::invalid_argument("rank must be in [0, 64)");
  hipLaunchKernelGGL(xgmi_fill_kernel, dim3(grid), dim3(XGMI_WG), 0, stream, buf, count, rank, seed);
  AK_HIP(hipGetLastError());
}

// waits for `stream`
inline XgmiCount xgmi_count_wrong_device(const float* buf, size_t count, int ranks, uint32_t seed, int grid, hipStream_t stream) {
  xgmi_check_ranks(ranks);
  DevBuf wrong(sizeof(unsigned long long)), nrec(sizeof(unsigned)), recs(XGMI_RECORDS * sizeof(XgmiRecord));
  AK_HIP(hipMemsetAsync(wrong.p, 0, wrong.bytes, stream));   // on the stream of the kernel: it may be a non-blocking one
  AK_HIP(hipMemsetAsync(nrec.p, 0, nrec.bytes, stream));
  hipLaunchKernelGGL(xgmi_count_kernel, dim3(grid), dim3(XGMI_WG), 0, stream, buf, count, ranks, seed,
                     wrong.as<unsigned long long>(), nrec.as<unsigned>(), recs.as<XgmiRecord>());
  AK_HIP(hipGetLastError());
  AK_HIP(hipStreamSynchronize(stream));
  XgmiCount r;
  r.wrong = wrong.download<unsigned long long>()[0];
  r.records = fetch_records<XgmiRecord>(nrec, recs);
  return r;
}

// flips the elements at `positions`, which must be distinct; waits for `stream`
inline void xgmi_flip_device(float* buf, size_t count, const std::vector<uint32_t>& positions, hipStream_t stream) {
  if (positions.size() > static_cast<size_t>(XGMI_MAX_FLIPS)) throw std::invalid_argument("at most 64 flips");
  for (uint32_t p : positions)
    if (p >= count) throw std::invalid_argument("a flip position lies past the buffer");
  if (positions.empty()) return;
  DevBuf pos(positions);
  hipLaunchKernelGGL(xgmi_flip_kernel, dim3(1), dim3(64), 0, stream, buf, count, pos.as<const uint32_t>(),
                     static_cast<int>(positions.size()));
  AK_HIP(hipGetLastError());
  AK_HIP(hipStreamSynchronize(stream));   // pos is freed on return
}

// ---- on host data, for the tests: `grid` 0 takes the production grid (host_grid of gpu_common.h)
// what rank `rank` contributes to an all-reduce of `count` elements
inline std::vector<float> xgmi_fill_host(size_t count, int rank, uint32_t seed, int dev, int grid = 0) {
  if (rank < 0 || rank >= XGMI_MAX_RANKS) throw std::invalid_argument("rank must be in [0, 64)");
  grid = host_grid(grid, XGMI_GRID);
  AK_HIP(hipSetDevice(dev));
  DevBuf d(count * sizeof(float));
  d.fill(0xff);   // NaN: an element the kernel skipped cannot pass
  xgmi_fill_device(d.as<float>(), count, rank, seed, grid, nullptr);
  return d.download<float>();
}

// the elements of `values` that are not the sum over `ranks` ranks, and the first of them
inline XgmiCount xgmi_count_wrong_host(const std::vector<float>& values, int ranks, uint32_t seed, int dev, int grid = 0) {
  xgmi_check_ranks(ranks);
  grid = host_grid(grid, XGMI_GRID);
  AK_HIP(hipSetDevice(dev));
  DevBuf d(values);
  return xgmi_count_wrong_device(d.as<const float>(), values.size(), ranks, seed, grid, nullptr);
}

}  // namespace amdkube
