// Checked matrix-core workload: a 64x64 bf16 MFMA tile staged through LDS, a GEMM on caller data
// (the numerics surface of the tests) and the integrity check behind mfma-check, gpu-burn --verify
// and the device plugin's mfma health probe. gpu_common.h provides mix32, bf16x8 / f32x16 and the
// host plumbing. The run type and its driver serve every format: mfma_check_lp.h adds the FP8 and MX
// kernels and the dispatch over formats; this header alone is the bf16 check (gpu-burn --verify).
//
// The check is the gpu-burn scheme anchored to an exact reference: every workgroup multiplies its
// own hashed integer operands, compares round 0 against int32 VALU arithmetic bit for bit, then
// recomputes the same product round after round and compares each result bitwise with round 0.
// A CU whose matrix cores return wrong products without raising an ECC event shows up as a
// non-zero error count. All loops are bounded, there is no inter-workgroup synchronisation and
// every __syncthreads sits in uniform control flow.
#pragma once

#include "gpu_common.h"

namespace amdkube {

constexpr int MFMA_TILE = 64;         // C tile edge: four waves, one 32x32 quadrant each
constexpr int MFMA_KSLICE = 64;       // K extent of one LDS slice of the GEMM
// LDS rows are padded by one 16-byte access, so a row is an odd number of 16-byte slots
// (K a multiple of 16) and the 16 lanes of a ds_read_b128 group, which read 16 distinct rows at
// one k offset, fall on 16 distinct slots of the 256-byte bank row: conflict-free.
constexpr int MFMA_PAD = 8;
constexpr int MFMA_CHECK_KMAX = 128;  // 2 x 64 x 136 bf16 = 34 KiB of LDS: four workgroups per CU
constexpr int MFMA_CHECK_BLOCKS_PER_CU = 4;
constexpr int MFMA_CHECK_RECORDS = 16;
constexpr int MFMA_CHECK_MAX_FLIPS = 4096;

// One K-slice of the 64x64 tile, operands already in LDS: As[i][k] = A[i][k] and Bt[j][k] = B[k][j],
// both with row stride ld (bf16 elements, a multiple of 8). Wave w owns the quadrant at rows
// 32(w>>1), columns 32(w&1). Lane maps as documented at mfma_tile_kernel: lane l, r = l&31,
// h = l>>5 feeds A[r][8h+j] and B[8h+j][r] per 16-deep step, 16 contiguous bytes each in these
// images (one ds_read_b128), and accumulator register q is C[(q&3) + 8(q>>2) + 4h][r].
__device__ __forceinline__ f32x16 mfma_tile64_slice(const __bf16* As, const __bf16* Bt, int ld, int k_steps, f32x16 acc) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
  const __bf16* ap = As + (32 * (w >> 1) + r) * ld + 8 * h;
  const __bf16* bp = Bt + (32 * (w & 1) + r) * ld + 8 * h;
  for (int ks = 0; ks < k_steps; ++ks) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + 16 * ks);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(bp + 16 * ks);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// tile row of accumulator register q for this lane's wave and half
__device__ __forceinline__ int mfma_tile64_row(int q) {
  const int w = threadIdx.x >> 6, h = (threadIdx.x >> 5) & 1;
  return 32 * (w >> 1) + (q & 3) + 8 * (q >> 2) + 4 * h;
}
__device__ __forceinline__ int mfma_tile64_col() { return 32 * ((threadIdx.x >> 6) & 1) + (threadIdx.x & 31); }

// C[MxN] fp32 = A[MxK] bf16 * B[KxN] bf16, all row-major; one workgroup per 64x64 tile of C,
// M and N multiples of 64, K a multiple of 16 (checked by mfma_gemm_host).
__global__ __launch_bounds__(256) void mfma_gemm_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                        float* __restrict__ C, int M, int N, int K) {
  constexpr int LD = MFMA_KSLICE + MFMA_PAD;
  __shared__ __attribute__((aligned(16))) __bf16 As[MFMA_TILE * LD];
  __shared__ __attribute__((aligned(16))) __bf16 Bt[MFMA_TILE * LD];
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += MFMA_KSLICE) {
    const int kk = K - k0 < MFMA_KSLICE ? K - k0 : MFMA_KSLICE;  // a multiple of 16
    // A slice: 64 rows x kk/8 16-byte chunks, copied as they lie
    for (int c = t; c < MFMA_TILE * (MFMA_KSLICE / 8); c += 256) {
      const int row = c >> 3, kc = (c & 7) * 8;
      if (kc < kk)
        *reinterpret_cast<bf16x8*>(As + row * LD + kc) =
            *reinterpret_cast<const bf16x8*>(A + (m0 + row) * K + k0 + kc);
    }
    // B slice, transposed: wave w takes k rows 16w..16w+15, lane l column l (128 contiguous bytes per row)
    const int kb = 16 * w;
    if (kb < kk) {
      bf16x8 lo, hi;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        lo[j] = B[static_cast<size_t>(k0 + kb + j) * N + n0 + l];
        hi[j] = B[static_cast<size_t>(k0 + kb + 8 + j) * N + n0 + l];
      }
      *reinterpret_cast<bf16x8*>(Bt + l * LD + kb) = lo;
      *reinterpret_cast<bf16x8*>(Bt + l * LD + kb + 8) = hi;
    }
    __syncthreads();
    acc = mfma_tile64_slice(As, Bt, LD, kk / 16, acc);
    __syncthreads();
  }
  const size_t col = n0 + mfma_tile64_col();
#pragma unroll
  for (int q = 0; q < 16; ++q) C[(m0 + mfma_tile64_row(q)) * N + col] = acc[q];
}

struct MfmaCheckRecord {
  uint32_t block, row, col, round, got, want;
};

// operand value: an integer in [-8, 8], exact in bf16
__device__ __forceinline__ float mfma_check_value(uint32_t seed, uint32_t block, uint32_t index) {
  return static_cast<float>(static_cast<int>(mix32(seed, block, index) % 17u) - 8);
}

// Self-test flips of round `round` that land on this lane, as a mask over its 16 accumulator
// registers. Flip i sits at tile position flip_pos[i] = block * 4096 + row * 64 + col (distinct
// positions, chosen by the host) and in round i mod rounds.
__device__ __forceinline__ uint32_t mfma_check_flip_mask(int round, int rounds, int flips, const uint32_t* flip_pos) {
  uint32_t m = 0;
  const uint32_t w = threadIdx.x >> 6, h = (threadIdx.x >> 5) & 1;
  for (long long i = round; i < flips; i += rounds) {
    const uint32_t p = flip_pos[i], b = p >> 12, row = (p >> 6) & 63, col = p & 63;
    if (b == blockIdx.x && col == static_cast<uint32_t>(mfma_tile64_col()) && (row >> 5) == (w >> 1) &&
        ((row >> 2) & 1) == h)
      m |= 1u << ((row & 3) + 4 * ((row & 31) >> 3));
  }
  return m;
}

// Compare the 16 accumulator values of one round with `want`; flip_mask XORs the low mantissa bit
// of the compared copy only. Returns the number of mismatches; the first few go to the record buffer.
__device__ __forceinline__ unsigned mfma_check_compare(const f32x16& got, const f32x16& want, uint32_t flip_mask, int round,
                                                       unsigned* nrec, MfmaCheckRecord* recs, unsigned* mine) {
  uint32_t diff = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) diff |= __float_as_uint(got[q]) ^ ((flip_mask >> q) & 1u) ^ __float_as_uint(want[q]);
  if (diff == 0) return 0;  // the healthy path: one branch per round, none per value
  unsigned bad = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const uint32_t g = __float_as_uint(got[q]) ^ ((flip_mask >> q) & 1u), e = __float_as_uint(want[q]);
    if (g != e) {
      ++bad;
      if (*mine < MFMA_CHECK_RECORDS) {  // a lane asks for at most 16 slots however long it runs
        ++*mine;
        const unsigned slot = atomicAdd(nrec, 1u);
        if (slot < MFMA_CHECK_RECORDS)
          recs[slot] = MfmaCheckRecord{blockIdx.x, static_cast<uint32_t>(mfma_tile64_row(q)),
                                       static_cast<uint32_t>(mfma_tile64_col()), static_cast<uint32_t>(round), g, e};
      }
    }
  }
  return bad;
}

// k_total: a multiple of 16 in [16, MFMA_CHECK_KMAX]; rounds >= 1; flip_pos holds
// MFMA_CHECK_MAX_FLIPS entries. Every partial sum is an integer of magnitude <= 64 * k_total < 2^24, so the fp32 result is exact in any accumulation order.
// dbg_block >= 0: that workgroup also stores its A[64 x k], B[k x 64] and round-0 C[64 x 64] (tests only).
__global__ __launch_bounds__(256, 4) void mfma_check_kernel(uint32_t seed, int k_total, int rounds, int flips,
                                                         const uint32_t* __restrict__ flip_pos,
                                                         unsigned long long* __restrict__ errors,
                                                         unsigned* __restrict__ nrec, MfmaCheckRecord* __restrict__ recs,
                                                         int dbg_block, float* __restrict__ dbg_a, float* __restrict__ dbg_b,
                                                         float* __restrict__ dbg_c) {
  __shared__ __attribute__((aligned(16))) __bf16 As[MFMA_TILE * (MFMA_CHECK_KMAX + MFMA_PAD)];
  __shared__ __attribute__((aligned(16))) __bf16 Bt[MFMA_TILE * (MFMA_CHECK_KMAX + MFMA_PAD)];
  // uniform: never index past the LDS images or the flip table, never loop on a non-positive stride
  if (k_total < 16 || k_total > MFMA_CHECK_KMAX || k_total % 16 || rounds < 1 || flips > MFMA_CHECK_MAX_FLIPS) return;
  const int ld = k_total + MFMA_PAD, k_steps = k_total / 16, t = threadIdx.x;
  const uint32_t nb = static_cast<uint32_t>(MFMA_TILE * k_total);
  for (uint32_t idx = t; idx < nb; idx += 256) {
    const uint32_t i = idx / k_total, k = idx - i * k_total;
    As[i * ld + k] = static_cast<__bf16>(mfma_check_value(seed, blockIdx.x, idx));                      // A[i][k]
    Bt[i * ld + k] = static_cast<__bf16>(mfma_check_value(seed, blockIdx.x, nb + k * MFMA_TILE + i));  // B[k][i]
  }
  __syncthreads();
  const bool dbg = static_cast<int>(blockIdx.x) == dbg_block;
  if (dbg)
    for (uint32_t idx = t; idx < nb; idx += 256) {
      const uint32_t i = idx / k_total, k = idx - i * k_total;
      dbg_a[i * k_total + k] = static_cast<float>(As[i * ld + k]);
      dbg_b[k * MFMA_TILE + i] = static_cast<float>(Bt[i * ld + k]);
    }

  // round 0: the MFMA product against int32 VALU arithmetic on the same LDS operands
  const f32x16 anchor = mfma_tile64_slice(As, Bt, ld, k_steps, f32x16{});
  const int col = mfma_tile64_col();
  f32x16 want;
#pragma unroll
  for (int q = 0; q < 16; ++q) {  // one output at a time keeps the register count at four workgroups per CU
    const __bf16* ar = As + mfma_tile64_row(q) * ld;
    const __bf16* bc = Bt + col * ld;
    int ref = 0;
    for (int kc = 0; kc < k_total; kc += 8) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(ar + kc);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(bc + kc);
#pragma unroll
      for (int j = 0; j < 8; ++j) ref += static_cast<int>(static_cast<float>(a[j])) * static_cast<int>(static_cast<float>(b[j]));
    }
    want[q] = static_cast<float>(ref);
  }
  if (dbg) {
#pragma unroll
    for (int q = 0; q < 16; ++q) dbg_c[mfma_tile64_row(q) * MFMA_TILE + col] = anchor[q];
  }
  unsigned mine = 0;
  unsigned long long bad =
      mfma_check_compare(anchor, want, mfma_check_flip_mask(0, rounds, flips, flip_pos), 0, nrec, recs, &mine);

  // rounds 1..: re-read the operands, recompute, compare bitwise with the kept round-0 accumulator
  for (int round = 1; round < rounds; ++round) {
    asm volatile("" ::: "memory");  // the operands are read from LDS again, the product is not reused
    const f32x16 c = mfma_tile64_slice(As, Bt, ld, k_steps, f32x16{});
    bad += mfma_check_compare(c, anchor, mfma_check_flip_mask(round, rounds, flips, flip_pos), round, nrec,
                              recs, &mine);
  }
  if (bad) atomicAdd(errors, bad);  // one per lane that saw a mismatch: none on a healthy part
}

// ---------------------------------------------------------------------------- runners
// C[m x n] fp32 = A[m x k] * B[k x n] from bf16 bit patterns, row-major
inline std::vector<float> mfma_gemm_host(const std::vector<uint16_t>& a_bits, const std::vector<uint16_t>& b_bits, int m,
                                         int n, int k, int dev) {
  if (m <= 0 || n <= 0 || m % MFMA_TILE || n % MFMA_TILE)
    throw std::invalid_argument("M and N must be positive multiples of 64");
  if (k <= 0 || k % 16) throw std::invalid_argument("K must be a positive multiple of 16");
  const size_t tiles = static_cast<size_t>(m / MFMA_TILE) * (n / MFMA_TILE);
  if (tiles > 0x7fffffffu) throw std::invalid_argument("too many tiles for one launch");
  if (a_bits.size() != static_cast<size_t>(m) * k || b_bits.size() != static_cast<size_t>(k) * n)
    throw std::invalid_argument("A must be MxK and B KxN bf16");
  AK_HIP(hipSetDevice(dev));
  DevBuf da(a_bits), db(b_bits), dc(static_cast<size_t>(m) * n * sizeof(float));
  hipLaunchKernelGGL(mfma_gemm_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, da.as<const __bf16>(),
                     db.as<const __bf16>(), dc.as<float>(), m, n, k);
  AK_HIP(hipGetLastError());
  return dc.download<float>();
}

inline int mfma_check_blocks(int cu_count) { return (cu_count > 0 ? cu_count : 256) * MFMA_CHECK_BLOCKS_PER_CU; }

struct MfmaCheckResult {
  double ms = 0, tflops = 0;
  long long rounds = 0;
  int blocks = 0, k = 0;
  unsigned long long errors = 0;
  std::vector<MfmaCheckRecord> first_errors;
};

// Device buffers of one check and the launch of its format; errors and records accumulate over launches.
struct MfmaCheckRun {
  // queues one launch of a format's check kernel on the run's buffers
  using Kernel = void (*)(const MfmaCheckRun& run, int rounds, int flips, int dbg_block, float* dbg_a, float* dbg_b,
                          float* dbg_c);
  int blocks, k;
  uint32_t seed;
  Kernel kernel;
  DevBuf errors, nrec, recs, flip_pos;
  // flip positions: distinct tile positions block * 4096 + row * 64 + col
  MfmaCheckRun(int dev, uint32_t seed_, int k_total, Kernel kernel_)
      : blocks(mfma_check_blocks(dev_info(dev).cu_count)), k(k_total), seed(seed_), kernel(kernel_),
        errors(sizeof(unsigned long long), DevBuf::zeroed), nrec(sizeof(unsigned), DevBuf::zeroed),
        recs(MFMA_CHECK_RECORDS * sizeof(MfmaCheckRecord), DevBuf::zeroed),
        flip_pos(flip_positions(seed_, MFMA_CHECK_MAX_FLIPS, static_cast<unsigned long long>(blocks) * (MFMA_TILE * MFMA_TILE))) {}
  void launch(int rounds, int flips, int dbg_block = -1, float* dbg_a = nullptr, float* dbg_b = nullptr,
              float* dbg_c = nullptr) const {
    kernel(*this, rounds, flips, dbg_block, dbg_a, dbg_b, dbg_c);
    AK_HIP(hipGetLastError());
  }
};

inline void mfma_check_launch_bf16(const MfmaCheckRun& run, int rounds, int flips, int dbg_block, float* dbg_a, float* dbg_b,
                                   float* dbg_c) {
  hipLaunchKernelGGL(mfma_check_kernel, dim3(run.blocks), dim3(256), 0, 0, run.seed, run.k, rounds, flips,
                     run.flip_pos.as<const uint32_t>(), run.errors.as<unsigned long long>(), run.nrec.as<unsigned>(),
                     run.recs.as<MfmaCheckRecord>(), dbg_block, dbg_a, dbg_b, dbg_c);
}

// One check of `kernel`'s format at K = k. rounds > 0: one launch of exactly that many rounds.
// rounds <= 0: calibrated to ~target_ms (check_core.h; the self-test flips go into the last launch only).
inline MfmaCheckResult mfma_check_drive(MfmaCheckRun::Kernel kernel, int k, int rounds, double target_ms, int dev,
                                        uint32_t seed, int flips) {
  if (flips < 0 || flips > MFMA_CHECK_MAX_FLIPS) throw std::invalid_argument("selftest flips must be in [0, 4096]");
  AK_HIP(hipSetDevice(dev));
  MfmaCheckRun run(dev, seed, k, kernel);
  GpuTimer timer;
  const Calibrated c =
      calibrate([&](int r, int f) { return timer.time([&] { run.launch(r, f); }); }, 256, 1 << 26, rounds, target_ms, flips);
  MfmaCheckResult r;
  r.errors = run.errors.download<unsigned long long>()[0];
  r.first_errors = fetch_records<MfmaCheckRecord>(run.nrec, run.recs);
  r.ms = c.ms;
  r.rounds = c.rounds;
  r.blocks = run.blocks;
  r.k = k;
  // every round is a full MFMA product of the tile, round 0 included
  r.tflops = static_cast<double>(run.blocks) * c.rounds * (2.0 * MFMA_TILE * MFMA_TILE * k) / (c.ms * 1e9);
  return r;
}

inline int mfma_check_bf16_k(int k) {
  if (k < 16 || k > MFMA_CHECK_KMAX || k % 16) throw std::invalid_argument("k must be a multiple of 16 in [16, 128]");
  return k;
}

inline MfmaCheckResult run_mfma_check(int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu, int flips = 0,
                                      int k_total = MFMA_CHECK_KMAX) {
  return mfma_check_drive(mfma_check_launch_bf16, mfma_check_bf16_k(k_total), rounds, target_ms, dev, seed, flips);
}

struct MfmaCheckTile {
  int k = 0;
  std::vector<float> a, b, c;  // A[64 x k], B[k x 64], round-0 C[64 x 64] of one workgroup
};

// one launch of a single round with workgroup `block` storing its operands and product
inline MfmaCheckTile mfma_check_fetch_tile(MfmaCheckRun::Kernel kernel, int k, int block, uint32_t seed, int dev) {
  AK_HIP(hipSetDevice(dev));
  MfmaCheckRun run(dev, seed, k, kernel);
  if (block < 0 || block >= run.blocks) throw std::invalid_argument("block out of range");
  const size_t nab = static_cast<size_t>(MFMA_TILE) * k, nc = static_cast<size_t>(MFMA_TILE) * MFMA_TILE;
  DevBuf da(nab * sizeof(float)), db(nab * sizeof(float)), dc(nc * sizeof(float));
  run.launch(1, 0, block, da.as<float>(), db.as<float>(), dc.as<float>());
  return MfmaCheckTile{k, da.download<float>(), db.download<float>(), dc.download<float>()};
}

inline MfmaCheckTile mfma_check_tile_host(int block, uint32_t seed, int dev, int k_total = MFMA_CHECK_KMAX) {
  return mfma_check_fetch_tile(mfma_check_launch_bf16, mfma_check_bf16_k(k_total), block, seed, dev);
}

}  // namespace amdkube

