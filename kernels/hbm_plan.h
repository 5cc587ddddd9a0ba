// What hbm-check tests and in which pieces: the region (a size in MiB, or a share of the free memory),
// its split into chunks, the seed of a chunk's background, and the way from a chunk and slot back to a
// region offset and a 2 MiB page. Plain C++17 with no HIP include, so native/hbm_plan_selftest.cpp checks
// it on the CPU, plain and under ASan/UBSan; kernels/hbm_check.h launches what it plans.
//
// A slot is 16 bytes, a page 2 MiB = 131,072 slots (the granule the driver maps device memory in, and
// the unit an operator retires). The region is a whole number of pages; every chunk but the last is
// chunk_mib MiB, chunk_mib is even, so no page straddles two chunks, and no chunk has more than 2^32
// slots, so a slot number fits the 32 bits a record has for it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace amdkube {

constexpr unsigned long long HBM_SLOT_BYTES = 16;
constexpr unsigned long long HBM_PAGE_BYTES = 2ull << 20;
constexpr unsigned HBM_PAGE_SHIFT_SLOTS = 17;                        // slots per page = 2^17
constexpr unsigned long long HBM_CHUNK_MAX_SLOTS = 1ull << 32;
constexpr long long HBM_CHUNK_MIB_DEFAULT = 1024;
constexpr long long HBM_CHUNK_MIB_MAX = static_cast<long long>(HBM_CHUNK_MAX_SLOTS * HBM_SLOT_BYTES >> 20);   // 65,536
constexpr long long HBM_MIB_MAX = 1ll << 30;                         // 1 PiB: keeps mib << 20 far from overflow
constexpr double HBM_FREE_FRACTION_MAX = 0.95;
// left to the counters, the records, the per-page array and the runtime's own allocations
constexpr unsigned long long HBM_PLAN_RESERVE_BYTES = 16ull << 20;
static_assert(HBM_PAGE_BYTES / HBM_SLOT_BYTES == 1ull << HBM_PAGE_SHIFT_SLOTS, "slots per page");

struct HbmPlan {
  unsigned long long bytes = 0;               // the region: a whole number of pages
  unsigned long long chunk_bytes = 0;         // of every chunk but the last
  std::vector<unsigned long long> chunks;     // bytes of each chunk, in region order
  unsigned long long pages() const { return bytes / HBM_PAGE_BYTES; }
};

// The part of hbm_plan that needs no device: mib == 0 and free_fraction == 0 mean "not given", and
// exactly one of them must be. Throws std::invalid_argument.
inline void hbm_plan_check_args(long long mib, double free_fraction, long long chunk_mib) {
  const bool has_mib = mib != 0, has_fraction = free_fraction != 0;   // NaN != 0: caught by the range below
  if (has_mib == has_fraction)
    throw std::invalid_argument(has_mib ? "give the region as --mib or as --free-fraction, not both"
                                        : "give the region as --mib or as --free-fraction");
  if (has_mib && (mib < 2 || mib > HBM_MIB_MAX)) throw std::invalid_argument("mib must be at least 2 (one 2 MiB page)");
  if (has_fraction && !(free_fraction > 0 && free_fraction <= HBM_FREE_FRACTION_MAX))
    throw std::invalid_argument("free fraction must be in (0, 0.95]");
  if (chunk_mib < 2 || chunk_mib % 2 || chunk_mib > HBM_CHUNK_MIB_MAX)
    throw std::invalid_argument("chunk mib must be even (whole 2 MiB pages), in [2, 65536] (at most 2^32 slots)");
}

// The chunks of the region that `mib` or `free_fraction` of `free_bytes` selects. Throws
// std::invalid_argument for what hbm_plan_check_args refuses, for a region under one page, and for one
// that does not fit `free_bytes` with HBM_PLAN_RESERVE_BYTES to spare: before anything is allocated.
inline HbmPlan hbm_plan(unsigned long long free_bytes, long long mib, double free_fraction,
                        long long chunk_mib = HBM_CHUNK_MIB_DEFAULT) {
  hbm_plan_check_args(mib, free_fraction, chunk_mib);
  unsigned long long want;
  if (mib != 0) {
    want = static_cast<unsigned long long>(mib) << 20;
  } else {
    const long double share = static_cast<long double>(free_bytes) * static_cast<long double>(free_fraction);
    want = static_cast<unsigned long long>(share);   // fraction <= 0.95: below free_bytes, no overflow
  }
  HbmPlan p;
  p.bytes = want / HBM_PAGE_BYTES * HBM_PAGE_BYTES;
  if (p.bytes < HBM_PAGE_BYTES) throw std::invalid_argument("the region is smaller than one 2 MiB page");
  if (free_bytes < HBM_PLAN_RESERVE_BYTES || p.bytes > free_bytes - HBM_PLAN_RESERVE_BYTES)
    throw std::invalid_argument("a region of " + std::to_string(p.bytes >> 20) + " MiB does not fit the " +
                                std::to_string(free_bytes >> 20) + " MiB free on the device (16 MiB are kept back)");
  p.chunk_bytes = static_cast<unsigned long long>(chunk_mib) << 20;
  for (unsigned long long at = 0; at < p.bytes; at += p.chunk_bytes)
    p.chunks.push_back(p.bytes - at < p.chunk_bytes ? p.bytes - at : p.chunk_bytes);
  return p;
}

// ---- from a chunk and slot back to the region
inline unsigned long long hbm_region_offset(const HbmPlan& p, uint32_t chunk, uint32_t slot) {
  return chunk * p.chunk_bytes + slot * HBM_SLOT_BYTES;
}
inline unsigned long long hbm_page_of(unsigned long long region_offset) { return region_offset / HBM_PAGE_BYTES; }
inline uint32_t hbm_chunk_of_page(const HbmPlan& p, unsigned long long page) {
  return static_cast<uint32_t>(page * HBM_PAGE_BYTES / p.chunk_bytes);
}
// the first page of a chunk: where the kernel's per-page counters of that chunk start
inline unsigned long long hbm_first_page(const HbmPlan& p, uint32_t chunk) { return chunk * p.chunk_bytes / HBM_PAGE_BYTES; }

// ---- the seed of one chunk's background in one round: mix32(seed, round, chunk) of gpu_common.h on the
// host, so two chunks, or two rounds, never expect the same data at the same slot
inline uint32_t hbm_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
inline uint32_t hbm_chunk_seed(uint32_t seed, uint32_t round, uint32_t chunk) {
  return hbm_mix32(hbm_mix32(seed ^ (0x9e3779b9u * (round + 1))) + chunk);
}

}  // namespace amdkube
