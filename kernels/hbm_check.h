// HBM integrity check: a MATS++ march over a region of device memory that compares every word it reads and
// says where an error sits. Behind hbm-check, the device plugin's --hbm-check-mib and hip.hbm_check.
// gpu_common.h provides the pattern, the streaming idiom (chunk_of, ld_nt / st_nt, HBM_UNROLL), the write
// kernel and the location words; hbm_plan.h the region, its chunks and the way back to an offset.
//
// The background is P(i) = pattern_v(i, seed_c), i the 16-byte slot within its chunk and
// seed_c = hbm_chunk_seed(seed, round, chunk): address-dependent, so a slot that aliases another one reads
// data nobody expects there. One round is four elements, each over the whole region before the next
// starts (a slot's write and its next read are a region apart):
//   E0  up    write P                          (hbm_write_kernel, pass 0)
//   E1  up    read, expect P,  write ~P        (pass 1)
//   E2  down  read, expect ~P, write P         (pass 2)
//   E3  down  read, expect P                   (pass 3)
// so every bit is read in both states and after both transitions. "down" runs the chunks from the last
// to the first and every workgroup's share from its top slot downwards.
//
// hbm_march_kernel is E1..E3: 256 lanes, each workgroup owns chunk_of its range, HBM_UNROLL non-temporal
// 16-byte loads in flight before the first compare, then a tail loop, as hbm_verify_kernel. The expected
// value is recomputed from the index and never loaded; what is stored is the complement of the EXPECTED
// value, not of the value read, so a fault shows once and is not carried into the next element. Every
// loop is bounded by the checked size and there is no inter-workgroup synchronisation.
//
// A mismatching slot takes hbm_march_mismatch, out of line: it loads the slot once more (`again`, before
// the element's own store) and, for each wrong 32-bit word, adds to errors, bit_errors (the popcount of
// got ^ want), transient (again == want) or persistent, and the counter of the slot's 2 MiB page, and
// keeps one of at most 64 records with the raw HW_ID / XCC_ID words of the wave that read it. The second
// load is an ordinary one: it says what the memory system delivers the second time, which for a line the
// first load left in a cache is that cache's copy.
//
// hbm_flip_kernel is the self-test: real corruption of the check's own buffer, one bit of one word in each
// of N slots of chunk 0, written with ordinary vector stores between E1 and E2 of round 0.
#pragma once

#include <chrono>
#include <memory>
#include <thread>

#include "gpu_common.h"
#include "hbm_plan.h"

namespace amdkube {

constexpr int HBM_CHECK_RECORDS = 64;
constexpr int HBM_CHECK_MAX_FLIPS = HBM_CHECK_RECORDS;   // so the self-test never drops a record
constexpr int HBM_CHECK_BAD_PAGES = 32;
constexpr int HBM_CHECK_MAX_ROUNDS = 1000000;
constexpr int HBM_CHECK_MAX_HOLD_MS = 600000;
constexpr uint32_t HBM_FLIP_TAG = 0x464c4950u;   // "FLIP": the block argument of the self-test's bit hash
enum : int { HBM_ERRORS = 0, HBM_BIT_ERRORS = 1, HBM_TRANSIENT = 2, HBM_PERSISTENT = 3, HBM_COUNTERS = 4 };

// slot is the 16-byte slot within its chunk, word the 32-bit word of the slot; got is what the march read,
// again what a second load of the same word gave
struct HbmCheckRecord {
  uint32_t round, pass, chunk, slot, word, got, want, again, hw_id, xcc_id;
};

struct HbmMarchTag {
  uint32_t round, pass, chunk;
};

struct HbmMarchOut {
  unsigned long long* counters;   // [HBM_COUNTERS]
  unsigned* page_errors;          // one per 2 MiB page of this chunk
  unsigned* nrec;
  HbmCheckRecord* recs;           // [HBM_CHECK_RECORDS]
};

// Out of line and by value: never taken on a healthy part, and it must not cost the march registers.
__device__ __noinline__ void hbm_march_mismatch(const v4u* p, uint32_t slot, v4u got, v4u want, HbmMarchTag tag,
                                                HbmMarchOut out) {
  const v4u again = *const_cast<const volatile v4u*>(p);
  const uint32_t hw_id = __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID), xcc_id = __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID);
#pragma unroll 1
  for (uint32_t c = 0; c < 4; ++c) {   // rolled up, with selects: small code on a path that is never taken
    const uint32_t g = c == 0 ? got.x : c == 1 ? got.y : c == 2 ? got.z : got.w;
    const uint32_t e = c == 0 ? want.x : c == 1 ? want.y : c == 2 ? want.z : want.w;
    const uint32_t a = c == 0 ? again.x : c == 1 ? again.y : c == 2 ? again.z : again.w;
    if (g == e) continue;
    atomicAdd(out.counters + HBM_ERRORS, 1ull);
    atomicAdd(out.counters + HBM_BIT_ERRORS, static_cast<unsigned long long>(__builtin_popcount(g ^ e)));
    atomicAdd(out.counters + (a == e ? HBM_TRANSIENT : HBM_PERSISTENT), 1ull);
    atomicAdd(out.page_errors + (slot >> HBM_PAGE_SHIFT_SLOTS), 1u);
    const unsigned at = atomicAdd(out.nrec, 1u);   // counts every request; the host reports the overflow
    if (at < static_cast<unsigned>(HBM_CHECK_RECORDS))
      out.recs[at] = HbmCheckRecord{tag.round, tag.pass, tag.chunk, slot, c, g, e, a, hw_id, xcc_id};
  }
}

// one slot: compare with P ^ inv, then (kWrite) store its complement
template <bool kWrite>
__device__ __forceinline__ void hbm_march_slot(v4u* p, size_t i, v4u got, uint32_t seed, uint32_t inv, HbmMarchTag tag,
                                               const HbmMarchOut& out) {
  const v4u want = pattern_v(i, seed) ^ inv;
  const v4u d = got ^ want;
  if (__builtin_expect((d.x | d.y | d.z | d.w) != 0, 0))   // the healthy path: one branch per slot
    hbm_march_mismatch(p, static_cast<uint32_t>(i), got, want, tag, out);
  if (kWrite) st_nt(p, ~want);
}

// kDown: lane t of a workgroup visits hi-1-t, hi-1-t-256, ... of its share [lo, hi) instead of lo+t,
// lo+t+256, ...: the same main / tail split over the distance from the end the walk starts at.
// n16 <= 2^32 (hbm_plan.h), so a slot number fits a record's 32 bits.
template <bool kDown, bool kWrite>
__global__ __launch_bounds__(256) void hbm_march_kernel(v4u* __restrict__ buf, size_t n16, uint32_t seed, uint32_t inv,
                                                        HbmMarchTag tag, HbmMarchOut out) {
  size_t lo, hi;
  chunk_of(n16, &lo, &hi);
  if (lo >= hi) return;   // an empty share: lo may lie past n16
  const size_t b = blockDim.x, len = hi - lo;
  auto at = [&](size_t d) { return kDown ? hi - 1 - d : lo + d; };   // d < len
  size_t d = threadIdx.x;
  for (; d + (HBM_UNROLL - 1) * b < len; d += HBM_UNROLL * b) {
    v4u v[HBM_UNROLL];
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) v[u] = ld_nt(buf + at(d + u * b));
#pragma unroll
    for (int u = 0; u < HBM_UNROLL; ++u) hbm_march_slot<kWrite>(buf + at(d + u * b), at(d + u * b), v[u], seed, inv, tag, out);
  }
  for (; d < len; d += b) hbm_march_slot<kWrite>(buf + at(d), at(d), ld_nt(buf + at(d)), seed, inv, tag, out);
}

// flip f < n: slots[f] of the n16 slots; h = mix32(seed, HBM_FLIP_TAG, f) picks word h & 3 and bit (h >> 2) & 31
__global__ __launch_bounds__(64) void hbm_flip_kernel(v4u* __restrict__ buf, size_t n16, const uint32_t* __restrict__ slots,
                                                      int n, uint32_t seed) {
  const int f = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
  if (f >= n || f >= HBM_CHECK_MAX_FLIPS) return;
  const uint32_t slot = slots[f];
  if (slot >= n16) return;
  const uint32_t h = mix32(seed, HBM_FLIP_TAG, static_cast<uint32_t>(f));
  reinterpret_cast<uint32_t*>(buf)[static_cast<size_t>(slot) * 4 + (h & 3u)] ^= 1u << ((h >> 2) & 31u);
}

// ---------------------------------------------------------------------------- runners
inline void hbm_march_launch(bool down, bool write, int grid, v4u* buf, size_t n16, uint32_t seed, uint32_t inv,
                             HbmMarchTag tag, const HbmMarchOut& out) {
  if (n16 == 0 || n16 > HBM_CHUNK_MAX_SLOTS) throw std::invalid_argument("a march launch takes 1 to 2^32 slots");
  auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, 0, buf, n16, seed, inv, tag, out); };
  if (down) {
    if (write) go(hbm_march_kernel<true, true>); else go(hbm_march_kernel<true, false>);
  } else {
    if (write) go(hbm_march_kernel<false, true>); else go(hbm_march_kernel<false, false>);
  }
  AK_HIP(hipGetLastError());
}

// the counters, per-page counters and records of a check, and what the host reads out of them
struct HbmCheckState {
  DevBuf counters, pages, nrec, recs;
  explicit HbmCheckState(size_t n_pages)
      : counters(HBM_COUNTERS * sizeof(unsigned long long), DevBuf::zeroed), pages(n_pages * sizeof(unsigned), DevBuf::zeroed),
        nrec(sizeof(unsigned), DevBuf::zeroed), recs(HBM_CHECK_RECORDS * sizeof(HbmCheckRecord), DevBuf::zeroed) {}
  HbmMarchOut out(size_t first_page) const {
    return HbmMarchOut{counters.as<unsigned long long>(), pages.as<unsigned>() + first_page, nrec.as<unsigned>(),
                       recs.as<HbmCheckRecord>()};
  }
};

struct HbmBadPage {
  unsigned long long offset = 0;   // of the page in the region
  uint32_t chunk = 0;
  unsigned errors = 0;
};

struct HbmCheckResult {
  unsigned long long bytes = 0;
  std::vector<unsigned long long> chunks;
  int rounds = 0, flips = 0, hold_ms = 0;
  double ms = 0, alloc_ms = 0, march_gbps = 0;
  unsigned long long errors = 0, bit_errors = 0, transient = 0, persistent = 0, records_dropped = 0;
  std::vector<HbmBadPage> bad_pages;   // at most HBM_CHECK_BAD_PAGES
  unsigned long long bad_pages_total = 0;
  std::vector<HbmCheckRecord> first_errors;
};

inline void hbm_check_read_counts(const HbmCheckState& st, HbmCheckResult* r) {
  const std::vector<unsigned long long> c = st.counters.download<unsigned long long>();
  r->errors = c[HBM_ERRORS];
  r->bit_errors = c[HBM_BIT_ERRORS];
  r->transient = c[HBM_TRANSIENT];
  r->persistent = c[HBM_PERSISTENT];
  const unsigned asked = st.nrec.download<unsigned>()[0];
  r->records_dropped = asked > static_cast<unsigned>(HBM_CHECK_RECORDS) ? asked - HBM_CHECK_RECORDS : 0;
  r->first_errors = fetch_records<HbmCheckRecord>(st.nrec, st.recs);
}

// free device memory as the plan wants it
inline unsigned long long hbm_free_bytes(int dev) {
  AK_HIP(hipSetDevice(dev));
  size_t free_b = 0, total_b = 0;
  AK_HIP(hipMemGetInfo(&free_b, &total_b));
  return free_b;
}

// `rounds` rounds of the march over the plan's region. flips > 0: the self-test corrupts that many slots
// of chunk 0 between E1 and E2 of round 0. hold_ms: a host sleep between E1 and E2 of every round (a
// retention wait), not counted into ms. Every buffer is a DevBuf: a thrown AK_HIP frees them all.
inline HbmCheckResult run_hbm_check(const HbmPlan& plan, int rounds, uint32_t seed, int flips, int hold_ms, int dev) {
  if (rounds < 1 || rounds > HBM_CHECK_MAX_ROUNDS) throw std::invalid_argument("rounds must be in [1, 1000000]");
  if (flips < 0 || flips > HBM_CHECK_MAX_FLIPS) throw std::invalid_argument("selftest flips must be in [0, 64]");
  if (hold_ms < 0 || hold_ms > HBM_CHECK_MAX_HOLD_MS) throw std::invalid_argument("hold ms must be in [0, 600000]");
  if (plan.chunks.empty()) throw std::invalid_argument("an empty plan");
  for (unsigned long long c : plan.chunks)
    if (c == 0 || c % HBM_PAGE_BYTES || c / HBM_SLOT_BYTES > HBM_CHUNK_MAX_SLOTS || c > plan.chunk_bytes)
      throw std::invalid_argument("a chunk is a whole number of 2 MiB pages, at most 2^32 slots");
  AK_HIP(hipSetDevice(dev));
  const int cus = dev_info(dev).cu_count;
  const uint32_t n_chunks = static_cast<uint32_t>(plan.chunks.size());
  HbmCheckResult r;
  r.bytes = plan.bytes;
  r.chunks = plan.chunks;
  r.rounds = rounds;
  r.flips = flips;
  r.hold_ms = hold_ms;

  const auto t_alloc = std::chrono::steady_clock::now();
  std::vector<std::unique_ptr<DevBuf>> bufs;
  for (unsigned long long c : plan.chunks) bufs.push_back(std::make_unique<DevBuf>(static_cast<size_t>(c)));
  r.alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc).count();
  HbmCheckState st(plan.pages());
  const size_t n16_first = plan.chunks[0] / HBM_SLOT_BYTES;
  const DevBuf flip_slots(flip_positions(seed, static_cast<size_t>(flips), n16_first));

  GpuTimer timer;
  // one element over the whole region: the chunks in order, or from the last to the first
  auto element = [&](int round, uint32_t pass, bool down, uint32_t inv, bool write) {
    r.ms += timer.time([&] {
      for (uint32_t k = 0; k < n_chunks; ++k) {
        const uint32_t c = down ? n_chunks - 1 - k : k;
        const size_t n16 = plan.chunks[c] / HBM_SLOT_BYTES;
        const uint32_t seed_c = hbm_chunk_seed(seed, static_cast<uint32_t>(round), c);
        v4u* buf = bufs[c]->as<v4u>();
        if (pass == 0) {
          hipLaunchKernelGGL(hbm_write_kernel, dim3(write_front_grid(cus)), dim3(256), 0, 0, buf, n16, seed_c);
          AK_HIP(hipGetLastError());
        } else {
          hbm_march_launch(down, write, stream_grid(n16, cus, HBM_COPY_BLOCKS_PER_CU), buf, n16, seed_c, inv,
                           HbmMarchTag{static_cast<uint32_t>(round), pass, c}, st.out(hbm_first_page(plan, c)));
        }
      }
    });
  };
  for (int round = 0; round < rounds; ++round) {
    element(round, 0, false, 0u, true);
    element(round, 1, false, 0u, true);
    if (round == 0 && flips > 0) {
      hipLaunchKernelGGL(hbm_flip_kernel, dim3(1), dim3(64), 0, 0, bufs[0]->as<v4u>(), n16_first,
                         flip_slots.as<const uint32_t>(), flips, seed);
      AK_HIP(hipGetLastError());
    }
    if (hold_ms > 0) {
      AK_HIP(hipDeviceSynchronize());
      std::this_thread::sleep_for(std::chrono::milliseconds(hold_ms));
    }
    element(round, 2, true, ~0u, true);
    element(round, 3, true, 0u, false);
  }
  hbm_check_read_counts(st, &r);
  r.march_gbps = r.ms > 0 ? 6.0 * static_cast<double>(plan.bytes) * rounds / (r.ms * 1e6) : 0;
  const std::vector<unsigned> pages = st.pages.download<unsigned>();
  for (size_t p = 0; p < pages.size(); ++p) {
    if (!pages[p]) continue;
    ++r.bad_pages_total;
    if (r.bad_pages.size() < static_cast<size_t>(HBM_CHECK_BAD_PAGES))
      r.bad_pages.push_back(HbmBadPage{p * HBM_PAGE_BYTES, hbm_chunk_of_page(plan, p), pages[p]});
  }
  return r;
}

// the plan for `mib` or `free_fraction` of the device's free memory, then the check
inline HbmCheckResult run_hbm_check(long long mib, double free_fraction, long long chunk_mib, int rounds, uint32_t seed,
                                    int flips, int hold_ms, int dev) {
  hbm_plan_check_args(mib, free_fraction, chunk_mib);   // before anything touches the GPU
  return run_hbm_check(hbm_plan(hbm_free_bytes(dev), mib, free_fraction, chunk_mib), rounds, seed, flips, hold_ms, dev);
}

// ---- one launch of the march kernel on caller data (bitwise against amdkube/ops/hbmcheck.py)
struct HbmMarchPassResult {
  std::vector<uint32_t> words, page_errors;
  HbmCheckResult counts;   // errors, bit_errors, transient, persistent, records_dropped, first_errors
};

inline HbmMarchPassResult hbm_march_pass_host(const std::vector<uint32_t>& words, uint32_t seed, uint32_t inv, bool down,
                                              bool write, int dev, int grid = 0) {
  if (words.empty() || words.size() % 4) throw std::invalid_argument("need a whole, positive number of 16-byte words");
  AK_HIP(hipSetDevice(dev));
  const size_t n16 = words.size() / 4;
  grid = host_grid(grid, stream_grid(n16, dev_info(dev).cu_count, HBM_COPY_BLOCKS_PER_CU));
  const size_t n_pages = (n16 + (size_t(1) << HBM_PAGE_SHIFT_SLOTS) - 1) >> HBM_PAGE_SHIFT_SLOTS;
  DevBuf d(words);
  HbmCheckState st(n_pages);
  hbm_march_launch(down, write, grid, d.as<v4u>(), n16, seed, inv, HbmMarchTag{0, 0, 0}, st.out(0));
  HbmMarchPassResult r;
  r.words = d.download<uint32_t>();
  r.page_errors = st.pages.download<unsigned>();
  hbm_check_read_counts(st, &r.counts);
  return r;
}

}  // namespace amdkube
