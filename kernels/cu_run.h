// The host side that the checks owning their CU share (cu_check.h, lane_check.h): a workgroup declares all
// 163,840 B of LDS, the grid is four workgroups per CU, and every launch leaves the error counts per unit and
// per workgroup, the first records and the raw HW_ID / XCC_ID words of where its workgroups ran. CuRun owns
// those buffers and what the launches have covered, cu_run() drives a check to its result. A check adds its
// kernel, its args struct, its flip table, its rates and what it counts as covered.
#pragma once

#include <type_traits>

#include "gpu_host.h"

namespace amdkube {

constexpr int CU_RUN_LDS_BYTES = 163840;
constexpr int CU_RUN_BLOCKS_PER_CU = 4;
constexpr int CU_RUN_RECORDS = 16;  // records and bad CUs kept

inline int cu_run_blocks(int cu_count) { return (cu_count > 0 ? cu_count : 256) * CU_RUN_BLOCKS_PER_CU; }

// what every per-CU result has; a check adds its rates (of the timed launch) and its own coverage figures
template <class Rec, int kUnits>
struct CuRunResult {
  double ms = 0;
  long long rounds = 0;
  int blocks = 0, units = 0, launches = 0;
  int cus = 0, cus_covered = 0, xccs = 0;
  unsigned long long errors = 0, errors_by_unit[kUnits] = {};
  std::vector<uint32_t> block_loc;   // the raw location words of every workgroup of the timed launch
  std::vector<CuBadCu> bad_cus;      // at most 16
  std::vector<Rec> first_errors;
};

// Device buffers and the launches of one check; errors and records accumulate over launches, the places and
// per-workgroup error counts are collected after each launch. `waves` is the number of HW_ID words a
// workgroup stores ahead of its XCC_ID, flip_table(seed, blocks, units) gives the self-test's positions.
struct CuRun {
  int cus, blocks, units;
  uint32_t seed;
  DevBuf errors, block_errors, nrec, recs, flip_pos, loc;
  CuCoverage coverage;
  std::vector<uint32_t> block_loc;
  int launches = 0;
  CuRun(const char* prog, int dev, uint32_t seed_, int units_, const char* const* names, int n_units, size_t rec_bytes,
        int waves, std::vector<uint32_t> (*flip_table)(uint32_t, int, int))
      : cus(dev_info(dev).cu_count), blocks(cu_run_blocks(cus)), units(checked_units(units_, names, n_units)), seed(seed_),
        errors(n_units * sizeof(unsigned long long), DevBuf::zeroed),
        block_errors(blocks * sizeof(unsigned), DevBuf::zeroed), nrec(sizeof(unsigned), DevBuf::zeroed),
        recs(CU_RUN_RECORDS * rec_bytes, DevBuf::zeroed), flip_pos(flip_table(seed_, blocks, units)),
        loc(static_cast<size_t>(blocks) * (waves + 1) * sizeof(uint32_t), DevBuf::zeroed), coverage(waves),
        block_loc(static_cast<size_t>(blocks) * (waves + 1)) {
    hipDeviceProp_t p;
    AK_HIP(hipGetDeviceProperties(&p, dev));
    if (p.sharedMemPerBlock < static_cast<size_t>(CU_RUN_LDS_BYTES))
      throw std::runtime_error(std::string(prog) + " needs 163840 bytes of LDS per workgroup, the device offers " +
                               std::to_string(p.sharedMemPerBlock));
  }
  static int checked_units(int units, const char* const* names, int n) {
    if (units < 1 || units >= 1 << n) throw std::invalid_argument("units must name at least one of " + unit_names(names, n));
    return units;
  }
  // the fields every args struct has
  template <class Args>
  Args args(int rounds, int flips) const {
    Args a = {};
    a.seed = seed;
    a.rounds = rounds;
    a.flips = flips;
    a.units = units;
    a.dbg_block = -1;
    a.flip_pos = flip_pos.as<const uint32_t>();
    a.errors = errors.as<unsigned long long>();
    a.block_errors = block_errors.as<unsigned>();
    a.nrec = nrec.as<unsigned>();
    a.recs = recs.as<std::remove_pointer_t<decltype(a.recs)>>();
    a.loc = loc.as<uint32_t>();
    return a;
  }
  template <class Args>
  void launch(void (*kernel)(Args), int threads, const Args& a) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, 0, a);
    AK_HIP(hipGetLastError());
    ++launches;
  }
  // after a finished launch: where its workgroups ran, and which of them counted errors
  void collect() {
    block_loc = loc.download<uint32_t>();
    if (coverage.add(block_loc, block_errors.download<unsigned>())) block_errors.zero();
  }
};

// Runs a check. rounds > 0: one launch of exactly that many rounds. rounds <= 0: calibrated to ~target_ms
// (check_core.h; the self-test flips go into the last launch only). While run.covered() is false, up to
// `extra_launches` launches of one round each are added (they check as well, and count into errors); the
// timed launch stays the reported one, with the places of its workgroups: run.finish(r, c) adds the check's
// rates from `c` and its own coverage figures.
template <class Result, class Run>
inline Result cu_run(Run& run, int rounds, double target_ms, int flips, int extra_launches) {
  GpuTimer timer;
  auto timed = [&](int r, int f) {
    const double ms = timer.time([&] { run.launch(run.args(r, f)); });
    run.collect();
    return ms;
  };
  const Calibrated c = calibrate(timed, 16, 1 << 26, rounds, target_ms, flips);
  Result r;
  r.block_loc = run.block_loc;
  for (int i = 0; i < extra_launches && !run.covered(); ++i) timed(1, 0);
  fetch_outcome(r, c, run.errors, run.nrec, run.recs);
  r.blocks = run.blocks;
  r.units = run.units;
  r.launches = run.launches;
  r.cus = run.cus;
  r.cus_covered = run.coverage.cus_covered();
  r.xccs = run.coverage.xccs();
  r.bad_cus = run.coverage.bad_cus(CU_RUN_RECORDS);
  run.finish(r, c);
  return r;
}

}  // namespace amdkube
