// Self-test of kernels/hbm_plan.h on the CPU (no HIP): the region and its chunks for sizes and shares of
// free memory, what is refused and that it is refused as std::invalid_argument, the way from a chunk and
// slot back to an offset and a page, the chunk seeds, and the self-test's slots. Built plain and
// with ASan/UBSan (native/build.py), run by tests/test_hbm_plan.py. Prints "OK ..." and exits 0, or says
// what failed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>
#include <set>

#include "../kernels/check_core.h"
#include "../kernels/hbm_plan.h"

using namespace amdkube;
using ull = unsigned long long;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);     \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

template <class F>
static bool refused(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

static ull sum(const HbmPlan& p) { return std::accumulate(p.chunks.begin(), p.chunks.end(), 0ull); }

// the invariants of every plan
static void check_plan(const HbmPlan& p, ull chunk_mib) {
  CHECK(p.bytes >= HBM_PAGE_BYTES && p.bytes % HBM_PAGE_BYTES == 0);
  CHECK(sum(p) == p.bytes && !p.chunks.empty());
  CHECK(p.chunk_bytes == chunk_mib << 20);
  for (size_t i = 0; i < p.chunks.size(); ++i) {
    CHECK(p.chunks[i] > 0 && p.chunks[i] % HBM_PAGE_BYTES == 0);
    CHECK(p.chunks[i] / HBM_SLOT_BYTES <= HBM_CHUNK_MAX_SLOTS);
    CHECK(i + 1 == p.chunks.size() ? p.chunks[i] <= p.chunk_bytes : p.chunks[i] == p.chunk_bytes);
  }
  CHECK(p.pages() * HBM_PAGE_BYTES == p.bytes);
}

int main() {
  const ull GiB = 1ull << 30, MiB = 1ull << 20, free288 = 288 * GiB;

  // ---- sizes
  {
    const HbmPlan p = hbm_plan(free288, 1024, 0);
    check_plan(p, 1024);
    CHECK(p.bytes == GiB && p.chunks.size() == 1);
  }
  {
    const HbmPlan p = hbm_plan(free288, 48, 0, 16);   // what the GPU tier runs
    check_plan(p, 16);
    CHECK(p.chunks == std::vector<ull>(3, 16 * MiB));
  }
  {
    const HbmPlan p = hbm_plan(free288, 2500, 0);     // a ragged last chunk
    check_plan(p, 1024);
    CHECK((p.chunks == std::vector<ull>{GiB, GiB, 452 * MiB}));
  }
  {
    const HbmPlan p = hbm_plan(free288, 3, 0);        // rounded down to whole pages
    check_plan(p, 1024);
    CHECK(p.bytes == 2 * MiB);
  }
  {
    const HbmPlan p = hbm_plan(free288, 7, 0, 2);     // one page per chunk
    check_plan(p, 2);
    CHECK(p.chunks == std::vector<ull>(3, 2 * MiB));
  }
  {
    const HbmPlan p = hbm_plan(free288, 200 * 1024, 0, 65536);   // the largest chunk: exactly 2^32 slots
    check_plan(p, 65536);
    CHECK(p.chunks.size() == 4 && p.chunks[0] / HBM_SLOT_BYTES == HBM_CHUNK_MAX_SLOTS && p.chunks[3] == 8 * GiB);
  }

  // ---- shares of free memory
  {
    const HbmPlan p = hbm_plan(free288, 0, 0.5);
    check_plan(p, 1024);
    CHECK(p.bytes == 144 * GiB && p.chunks.size() == 144);
  }
  {
    const ull free_odd = 287 * GiB + 12345678;
    const HbmPlan p = hbm_plan(free_odd, 0, 0.001);
    check_plan(p, 1024);
    const ull want = static_cast<ull>(static_cast<long double>(free_odd) * 0.001L);
    CHECK(p.bytes <= want && want - p.bytes < HBM_PAGE_BYTES);
  }
  {
    const HbmPlan p = hbm_plan(free288, 0, 0.95, 4096);
    check_plan(p, 4096);
    CHECK(p.bytes <= free288 - HBM_PLAN_RESERVE_BYTES);
  }

  // ---- refused, and as invalid_argument
  CHECK(refused([&] { hbm_plan(free288, 0, 0); }));              // neither
  CHECK(refused([&] { hbm_plan(free288, 48, 0.5); }));           // both
  CHECK(refused([&] { hbm_plan(free288, -1, 0); }));
  CHECK(refused([&] { hbm_plan(free288, 1, 0); }));              // under one page
  CHECK(refused([&] { hbm_plan(free288, HBM_MIB_MAX + 1, 0); }));
  CHECK(refused([&] { hbm_plan(free288, std::numeric_limits<long long>::min(), 0); }));
  CHECK(refused([&] { hbm_plan(free288, 0, 0.96); }));
  CHECK(refused([&] { hbm_plan(free288, 0, -0.5); }));
  CHECK(refused([&] { hbm_plan(free288, 0, std::nan("")); }));
  CHECK(refused([&] { hbm_plan(free288, 0, std::numeric_limits<double>::infinity()); }));
  CHECK(refused([&] { hbm_plan(free288, 48, 0, 0); }));
  CHECK(refused([&] { hbm_plan(free288, 48, 0, 3); }));          // a page would straddle two chunks
  CHECK(refused([&] { hbm_plan(free288, 48, 0, -2); }));
  CHECK(refused([&] { hbm_plan(free288, 48, 0, 65538); }));      // more than 2^32 slots
  CHECK(refused([&] { hbm_plan(free288, 288 * 1024, 0); }));     // all of it: nothing left for the counters
  CHECK(refused([&] { hbm_plan(free288, 300 * 1024, 0); }));
  CHECK(refused([&] { hbm_plan(0, 48, 0); }));
  CHECK(refused([&] { hbm_plan(MiB, 0, 0.5); }));                // half of 1 MiB is no page
  CHECK(refused([&] { hbm_plan(17 * MiB, 0, 0.95); }));          // 16 MiB do not leave the reserve
  CHECK(!refused([&] { hbm_plan(free288, 288 * 1024 - 16, 0); }));
  CHECK(refused([&] { hbm_plan_check_args(48, 0.5, 1024); }));
  CHECK(!refused([&] { hbm_plan_check_args(48, 0, 1024); }));

  // ---- offsets and pages
  {
    const HbmPlan p = hbm_plan(free288, 2500, 0);
    CHECK(hbm_region_offset(p, 0, 0) == 0 && hbm_region_offset(p, 2, 5) == 2 * GiB + 80);
    CHECK(hbm_region_offset(p, 1, 0xffffffffu) == GiB + 0xffffffffull * 16);   // no 32-bit wrap
    CHECK(hbm_page_of(hbm_region_offset(p, 0, 131071)) == 0 && hbm_page_of(hbm_region_offset(p, 0, 131072)) == 1);
    CHECK(hbm_page_of(hbm_region_offset(p, 2, 0)) == 1024 && hbm_first_page(p, 2) == 1024);
    CHECK(hbm_chunk_of_page(p, 1023) == 1 && hbm_chunk_of_page(p, 1024) == 2 && hbm_chunk_of_page(p, p.pages() - 1) == 2);
    // every page belongs to the chunk whose pages hbm_first_page starts
    for (ull page = 0; page < p.pages(); ++page) {
      const uint32_t c = hbm_chunk_of_page(p, page);
      CHECK(c < p.chunks.size() && hbm_first_page(p, c) <= page && page < hbm_first_page(p, c) + p.chunks[c] / HBM_PAGE_BYTES);
    }
    const HbmPlan big = hbm_plan(free288, 200 * 1024, 0, 65536);
    CHECK(hbm_region_offset(big, 3, 1) == 192 * GiB + 16 && hbm_first_page(big, 3) == 192 * 512);
  }

  // ---- seeds: distinct over rounds and chunks, and the hash itself against values worked by hand
  {
    CHECK(hbm_mix32(0) == 0 && hbm_mix32(1) == 0x688990c0u);
    std::set<uint32_t> seen;
    for (uint32_t round = 0; round < 16; ++round)
      for (uint32_t chunk = 0; chunk < 288; ++chunk) seen.insert(hbm_chunk_seed(0x5eedu, round, chunk));
    CHECK(seen.size() == 16 * 288);
    CHECK(hbm_chunk_seed(0x5eedu, 0, 0) != hbm_chunk_seed(0x5eeeu, 0, 0));
  }

  // ---- the self-test: distinct slots of chunk 0 for every count up to 64
  {
    for (uint32_t seed : {0x5eedu, 0xc0ffee11u, 0u, 0xffffffffu})
      for (ull n16 : {1ull << 17, 1ull << 20, 3ull << 17}) {
        for (size_t n = 0; n <= 64; ++n) {
          const std::vector<uint32_t> pos = flip_positions(seed, n, n16);
          const std::set<uint32_t> distinct(pos.begin(), pos.end());
          CHECK(pos.size() == n && distinct.size() == n);
          for (uint32_t s : pos) CHECK(s < n16);
        }
      }
  }

  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK hbm_plan: sizes, shares, refusals, offsets, seeds, flips\n");
  return 0;
}
