// Low-precision matrix-core check: the 64x64 tile, GEMM and integrity check of mfma_check.h for the
// FP8 and block-scaled MX paths of CDNA4, on the run type, driver, record buffer, flip mask and
// compare of mfma_check.h. mfma_fmt_ops is the one table from a format, bf16 included, to its kernels.
//
//   fp8    v_mfma_f32_32x32x16_fp8_fp8, OCP e4m3fn operands, K step 16
//   mxfp8  v_mfma_scale_f32_32x32x64_f8f6f4, cbsz = blgp = 0 (e4m3), one E8M0 scale per 32 k, K step 64
//   mxfp4  the same instruction, cbsz = blgp = 4 (e2m1, two codes per byte), K step 64
//
// Operand lane maps, as the kernels use them and as the one-hot and exact-GEMM tests of
// tests/test_gpu_mfma_lp.py check them on the part (lane l, r = l&31, h = l>>5):
//   fp8     byte j of the 64-bit operand is A[r][8h+j] and B[8h+j][r]
//   mxfp4   the low four registers of the operand hold the 32 consecutive k values 32h..32h+31 of
//           row (A) or column (B) r, lowest k in the lowest byte and there in the low nibble
//   mxfp8   registers 0-3 hold k = 16h..16h+15 and registers 4-7 hold k = 32+16h..32+16h+15, lowest k
//           in the lowest byte: a lane's bytes lie in both MX blocks of the step
//   scales  both scaled forms: lane (r, h) supplies the scale of block h of the step (k = 32h..32h+31)
//           of row or column r, in the byte of its scale register that opsel picks
// (With e4m3 operands in the e2m1 arrangement, 32 consecutive k per lane, every product that carried
// block scales came out wrong on the part: the scale of lane half h goes to block h of the step, not
// to the lane's own bytes. The e2m1 arrangement was right as first written.)
// The C/D map is the bf16 one (mfma_tile64_row / mfma_tile64_col).
#pragma once

#include "mfma_check.h"

namespace amdkube {

// MFMA_BF16 is the check of mfma_check.h, so that one list of formats serves mfma-check; it has no GEMM here
enum MfmaLpFmt { MFMA_LP_FP8 = 0, MFMA_LP_MXFP8 = 1, MFMA_LP_MXFP4 = 2, MFMA_BF16 = 3 };

typedef int lp_v4i __attribute__((ext_vector_type(4)));
typedef int lp_v8i __attribute__((ext_vector_type(8)));

constexpr int MFMA_LP_BLOCK = 32;        // k values per E8M0 scale
constexpr int MFMA_LP_GEMM_KSLICE = 128; // k values of one LDS slice of the GEMM
constexpr int MFMA_LP_SCALE_ONE = 127;   // E8M0 bias: byte e is 2^(e - 127)
constexpr int MFMA_LP_SCALE_MIN = 126;   // the check draws its scales from 2^-1, 1, 2

__host__ __device__ constexpr bool mfma_lp_scaled(int f) { return f != MFMA_LP_FP8; }
__host__ __device__ constexpr int mfma_lp_kstep(int f) { return f == MFMA_LP_FP8 ? 16 : 64; }
__host__ __device__ constexpr int mfma_lp_row_bytes(int f, int k) { return f == MFMA_LP_MXFP4 ? k / 2 : k; }
// K of the check: 256 B of LDS per operand row for the scaled formats, as the bf16 check has
__host__ __device__ constexpr int mfma_lp_check_kmax(int f) { return f == MFMA_LP_MXFP4 ? 512 : 256; }
// LDS row padding. An operand read takes all 32 rows of a lane half at one k offset.
//   fp8: one ds_read_b64 per operand, serviced per 32-lane half. The pad of 8 makes the row stride
//   an odd number of 8-byte slots (row bytes are a multiple of 16), so the 32 rows fall on the 32
//   distinct 8-byte slots of the 256-byte bank row: conflict-free.
//   scaled: ds_read_b128 (two per operand for e4m3, one for e2m1), serviced in groups of 16 lanes
//   whose rows are distinct mod 16. The pad of 16 makes the stride an odd number of 16-byte slots
//   (row bytes are a multiple of 32), so a group's 16 rows fall on the 16 distinct slots of the
//   bank row: conflict-free.
__host__ __device__ constexpr int mfma_lp_pad(int f) { return f == MFMA_LP_FP8 ? 8 : 16; }
__host__ __device__ constexpr int mfma_lp_ld(int f, int k) { return mfma_lp_row_bytes(f, k) + mfma_lp_pad(f); }

// Place of the E8M0 byte of (32-wide K block b, row or column i) in an LDS scale table. Block b
// belongs to K step b >> 1 and lane half b & 1; the bytes of four consecutive steps of one (half,
// row) share a dword, and the dwords of a half's 32 rows are consecutive (one conflict-free
// ds_read_b32 per operand and four steps). A table for n blocks holds 512 * ((n + 7) / 8) bytes.
__host__ __device__ constexpr int mfma_lp_scale_index(int b, int i) {
  return ((((b >> 3) * 2 + (b & 1)) * MFMA_TILE + i) << 2) + ((b >> 1) & 3);
}
__host__ __device__ constexpr int mfma_lp_scale_bytes(int blocks) { return 512 * ((blocks + 7) / 8); }

// One K-slice of the 64x64 tile from LDS row images in packed format bytes: As row i holds
// A[i][k], Bt row j holds B[k][j], both with row stride ld bytes. Wave w owns the quadrant at rows
// 32(w>>1), columns 32(w&1), as in mfma_tile64_slice.
__device__ __forceinline__ f32x16 mfma_fp8_tile64_slice(const uint8_t* As, const uint8_t* Bt, int ld, int k_steps,
                                                        f32x16 acc) {
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
  const uint8_t* ap = As + (32 * (w >> 1) + r) * ld + 8 * h;
  const uint8_t* bp = Bt + (32 * (w & 1) + r) * ld + 8 * h;
  for (int ks = 0; ks < k_steps; ++ks) {
    const long a = *reinterpret_cast<const long*>(ap + 16 * ks);
    const long b = *reinterpret_cast<const long*>(bp + 16 * ks);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// one scaled MFMA whose scales are byte j of swa and swb (opsel is an immediate)
template <int F>
__device__ __forceinline__ f32x16 mfma_mx_step(lp_v8i a, lp_v8i b, f32x16 acc, int j, int swa, int swb) {
  constexpr int FMT = F == MFMA_LP_MXFP8 ? 0 : 4;  // cbsz / blgp: e4m3 or e2m1
  switch (j) {
    case 0: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 0, swa, 0, swb);
    case 1: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 1, swa, 1, swb);
    case 2: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 2, swa, 2, swb);
    default: return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT, FMT, 3, swa, 3, swb);
  }
}

// The same for the scaled formats, STEPS K steps of 64, fully unrolled: sa / sb are scale tables laid
// out by mfma_lp_scale_index, read one dword per operand and four steps, the step's byte picked by opsel.
template <int F, int STEPS>
__device__ __forceinline__ f32x16 mfma_mx_tile64_slice(const uint8_t* As, const uint8_t* Bt, int ld, const uint8_t* sa,
                                                       const uint8_t* sb, f32x16 acc) {
  constexpr int STEP_BYTES = mfma_lp_row_bytes(F, 64);
  // e4m3 (16 operand registers a step, e2m1 has 8): the lane's four LDS addresses are worked out again
  // at every call, from a thread id the compiler cannot see through. Kept in registers across the
  // check's round loop they pushed that kernel past the 128 registers of four workgroups per CU
  // (24 dwords spilled); recomputing them costs 7 % of its rate (2375 against 2550 TFLOP/s).
  unsigned tid = threadIdx.x;
  if constexpr (F == MFMA_LP_MXFP8) asm volatile("" : "+v"(tid));
  const int l = tid & 63, w = tid >> 6, r = l & 31, h = l >> 5;
  const int ra = 32 * (w >> 1) + r, cb = 32 * (w & 1) + r;
  const uint8_t* ap = As + ra * ld + 16 * h;  // e2m1: k = 32h of the step; e4m3: k = 16h, and 32 + 16h below
  const uint8_t* bp = Bt + cb * ld + 16 * h;
  int swa = 0, swb = 0;
#pragma unroll
  for (int ks = 0; ks < STEPS; ++ks) {
    if (ks % 4 == 0) {
      swa = *reinterpret_cast<const int*>(sa + mfma_lp_scale_index(2 * ks, 0) + 4 * (h * MFMA_TILE + ra));
      swb = *reinterpret_cast<const int*>(sb + mfma_lp_scale_index(2 * ks, 0) + 4 * (h * MFMA_TILE + cb));
    }
    const lp_v4i a0 = *reinterpret_cast<const lp_v4i*>(ap + STEP_BYTES * ks);
    const lp_v4i b0 = *reinterpret_cast<const lp_v4i*>(bp + STEP_BYTES * ks);
    lp_v4i a1 = {}, b1 = {};  // e2m1 fills the low four registers only
    if constexpr (F == MFMA_LP_MXFP8) {
      a1 = *reinterpret_cast<const lp_v4i*>(ap + STEP_BYTES * ks + 32);
      b1 = *reinterpret_cast<const lp_v4i*>(bp + STEP_BYTES * ks + 32);
    }
    acc = mfma_mx_step<F>(__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7),
                          __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7), acc, ks % 4, swa, swb);
    asm volatile("" : "+v"(acc)::"memory");  // the next step's reads follow this product: one step's operands in registers
  }
  return acc;
}

// C[MxN] fp32 = A * B on caller codes, one workgroup per 64x64 tile of C. A is the M x row_bytes(K)
// image of A and Bt the N x row_bytes(K) image of B transposed, both in packed format bytes; SA is
// [K/32][M] and SB [K/32][N] E8M0 bytes (scaled formats only). M and N multiples of 64, K a multiple
// of the format's K step (checked by mfma_gemm_lp_host, which also packs and transposes).
template <int F>
__global__ __launch_bounds__(256) void mfma_gemm_lp_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bt,
                                                           const uint8_t* __restrict__ SA, const uint8_t* __restrict__ SB,
                                                           float* __restrict__ C, int M, int N, int K) {
  constexpr int LD = mfma_lp_ld(F, MFMA_LP_GEMM_KSLICE);
  constexpr int SLICE_BLOCKS = MFMA_LP_GEMM_KSLICE / MFMA_LP_BLOCK;
  constexpr int CHUNKS = mfma_lp_row_bytes(F, MFMA_LP_GEMM_KSLICE) / 8;  // 8-byte chunks per row slice
  __shared__ __attribute__((aligned(16))) uint8_t As[MFMA_TILE * LD];
  __shared__ __attribute__((aligned(16))) uint8_t Bs[MFMA_TILE * LD];
  constexpr int NSCALE = mfma_lp_scaled(F) ? mfma_lp_scale_bytes(SLICE_BLOCKS) : 4;
  __shared__ __attribute__((aligned(4))) uint8_t sa[NSCALE];
  __shared__ __attribute__((aligned(4))) uint8_t sb[NSCALE];
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x;
  const size_t rb = mfma_lp_row_bytes(F, K);
  f32x16 acc = {};
  for (int k0 = 0; k0 < K; k0 += MFMA_LP_GEMM_KSLICE) {
    const int kk = K - k0 < MFMA_LP_GEMM_KSLICE ? K - k0 : MFMA_LP_GEMM_KSLICE;  // a multiple of the K step
    const int kkb = mfma_lp_row_bytes(F, kk);                                      // a multiple of 16
    const size_t k0b = mfma_lp_row_bytes(F, k0);
    for (int c = t; c < MFMA_TILE * CHUNKS; c += 256) {
      const int row = c / CHUNKS, off = (c % CHUNKS) * 8;
      if (off < kkb) {
        *reinterpret_cast<uint2*>(As + row * LD + off) = *reinterpret_cast<const uint2*>(A + (m0 + row) * rb + k0b + off);
        *reinterpret_cast<uint2*>(Bs + row * LD + off) = *reinterpret_cast<const uint2*>(Bt + (n0 + row) * rb + k0b + off);
      }
    }
    if constexpr (mfma_lp_scaled(F)) {
      const int b = t >> 6, i = t & 63;  // 256 threads: SLICE_BLOCKS x 64 scale bytes per operand
      if (b * MFMA_LP_BLOCK < kk) {
        sa[mfma_lp_scale_index(b, i)] = SA[static_cast<size_t>(k0 / MFMA_LP_BLOCK + b) * M + m0 + i];
        sb[mfma_lp_scale_index(b, i)] = SB[static_cast<size_t>(k0 / MFMA_LP_BLOCK + b) * N + n0 + i];
      }
    }
    __syncthreads();
    if constexpr (F == MFMA_LP_FP8) acc = mfma_fp8_tile64_slice(As, Bs, LD, kk / 16, acc);
    else if (kk == MFMA_LP_GEMM_KSLICE) acc = mfma_mx_tile64_slice<F, MFMA_LP_GEMM_KSLICE / 64>(As, Bs, LD, sa, sb, acc);
    else acc = mfma_mx_tile64_slice<F, 1>(As, Bs, LD, sa, sb, acc);  // the last 64 of K
    __syncthreads();
  }
  const size_t col = n0 + mfma_tile64_col();
#pragma unroll
  for (int q = 0; q < 16; ++q) C[(m0 + mfma_tile64_row(q)) * N + col] = acc[q];
}

// ---- decode by bit arithmetic (no hardware conversion): fixed point, exact for every finite code
// e4m3fn code -> value * 2^9 (subnormals are m * 2^-9; |value| <= 448)
__device__ __forceinline__ int mfma_lp_e4m3_q9(uint32_t c) {
  const int e = (c >> 3) & 15, m = c & 7, v = e ? (8 + m) << (e - 1) : m;
  return c & 0x80 ? -v : v;
}
// e2m1 code -> value * 2 (0, 0.5, 1, 1.5, 2, 3, 4, 6)
__device__ __forceinline__ int mfma_lp_e2m1_q1(uint32_t c) {
  const int e = (c >> 1) & 3, m = c & 1, v = e ? (2 + m) << (e - 1) : m;
  return c & 8 ? -v : v;
}
template <int F>
__device__ __forceinline__ int mfma_lp_decode(const uint8_t* row, int k) {
  if constexpr (F == MFMA_LP_MXFP4) return mfma_lp_e2m1_q1((row[k >> 1] >> (4 * (k & 1))) & 15);
  else return mfma_lp_e4m3_q9(row[k]);
}
template <int F>
__host__ __device__ constexpr int mfma_lp_frac_bits() { return F == MFMA_LP_MXFP4 ? 1 : 9; }

// hashed operand codes of the check
//   fp8, mxfp8: the integers -15..15, all four significant bits of e4m3 in use
//   mxfp4: the 15 distinct e2m1 values (codes 0..7 and 9..15; 8 is -0)
template <int F>
__device__ __forceinline__ uint32_t mfma_lp_check_code(uint32_t seed, uint32_t block, uint32_t index) {
  const uint32_t x = mix32(seed, block, index);
  if constexpr (F == MFMA_LP_MXFP4) {
    const uint32_t c = x % 15u;
    return c < 8 ? c : c + 1;
  } else {
    const int v = static_cast<int>(x % 31u) - 15, n = v < 0 ? -v : v;
    if (n == 0) return 0;
    const int p = 31 - __clz(n);  // n = 1.mmm * 2^p, p <= 3
    return (v < 0 ? 0x80u : 0u) | static_cast<uint32_t>(p + 7) << 3 | (static_cast<uint32_t>(n << (3 - p)) & 7u);
  }
}
// hashed block scale of the check: 2^-1, 1 or 2
__device__ __forceinline__ uint8_t mfma_lp_check_scale(uint32_t seed, uint32_t block, uint32_t index) {
  return static_cast<uint8_t>(MFMA_LP_SCALE_MIN + mix32(seed, block, index) % 3u);
}

// the check's product of the tile in LDS
template <int F>
__device__ __forceinline__ f32x16 mfma_lp_check_product(const uint8_t* As, const uint8_t* Bt, const uint8_t* sa,
                                                        const uint8_t* sb) {
  constexpr int K = mfma_lp_check_kmax(F);
  if constexpr (F == MFMA_LP_FP8) return mfma_fp8_tile64_slice(As, Bt, mfma_lp_ld(F, K), K / 16, f32x16{});
  else return mfma_mx_tile64_slice<F, K / 64>(As, Bt, mfma_lp_ld(F, K), sa, sb, f32x16{});
}

// The check of mfma_check_kernel on format F, K = mfma_lp_check_kmax(F). rounds >= 1; flip_pos holds
// MFMA_CHECK_MAX_FLIPS entries.
// Why the comparison is bitwise: with u the smallest unit of a product (operand unit squared times the
// two smallest scales), every product and every partial sum is an integer multiple of u, and the check
// is exact in any accumulation order while |sum| / u < 2^24, because every such value is an fp32 number:
//   fp8    integers, u = 1:                              |sum| <= 15^2 * 256          = 5.8e4
//   mxfp8  integers times 2^-1..2, u = 2^-2:             |sum| / u <= 15^2 * 4 * 256 * 4 = 9.2e5
//   mxfp4  multiples of 1/2 times 2^-1..2, u = 2^-4:     |sum| / u <= 6^2 * 4 * 512 * 16 = 1.2e6
// The reference is integer arithmetic on the VALU, in units of u, from the bytes in LDS.
// dbg_block >= 0: that workgroup also stores its A[64 x k] and B[k x 64] decoded to fp32 with the
// scales applied, and its round-0 C[64 x 64] (tests only).
template <int F>
__global__ __launch_bounds__(256, 4) void mfma_check_lp_kernel(uint32_t seed, int rounds, int flips,
                                                               const uint32_t* __restrict__ flip_pos,
                                                               unsigned long long* __restrict__ errors,
                                                               unsigned* __restrict__ nrec, MfmaCheckRecord* __restrict__ recs,
                                                               int dbg_block, float* __restrict__ dbg_a,
                                                               float* __restrict__ dbg_b, float* __restrict__ dbg_c) {
  constexpr int KMAX = mfma_lp_check_kmax(F);
  constexpr int NSCALE = mfma_lp_scaled(F) ? mfma_lp_scale_bytes(KMAX / MFMA_LP_BLOCK) : 4;
  __shared__ __attribute__((aligned(16))) uint8_t As[MFMA_TILE * mfma_lp_ld(F, KMAX)];  // 2 x 64 x 272 B = 34 KiB at most
  __shared__ __attribute__((aligned(16))) uint8_t Bt[MFMA_TILE * mfma_lp_ld(F, KMAX)];
  __shared__ __attribute__((aligned(4))) uint8_t sa[NSCALE];                            // up to 2 x 1 KiB
  __shared__ __attribute__((aligned(4))) uint8_t sb[NSCALE];
  // uniform: never index past the flip table, never loop on a non-positive stride
  if (rounds < 1 || flips > MFMA_CHECK_MAX_FLIPS) return;
  constexpr int k_total = KMAX, rb = mfma_lp_row_bytes(F, k_total), ld = mfma_lp_ld(F, k_total);
  constexpr int kblocks = k_total / MFMA_LP_BLOCK;
  const int t = threadIdx.x;
  const uint32_t nb = static_cast<uint32_t>(MFMA_TILE * k_total);
  for (uint32_t idx = t; idx < static_cast<uint32_t>(MFMA_TILE * rb); idx += 256) {
    const uint32_t i = idx / rb, kb = idx - i * rb;
    if constexpr (F == MFMA_LP_MXFP4) {  // two codes per byte, the lower k in the low nibble
      const uint32_t k = 2 * kb;
      As[i * ld + kb] = static_cast<uint8_t>(mfma_lp_check_code<F>(seed, blockIdx.x, i * k_total + k) |
                                             mfma_lp_check_code<F>(seed, blockIdx.x, i * k_total + k + 1) << 4);
      Bt[i * ld + kb] = static_cast<uint8_t>(mfma_lp_check_code<F>(seed, blockIdx.x, nb + k * MFMA_TILE + i) |
                                             mfma_lp_check_code<F>(seed, blockIdx.x, nb + (k + 1) * MFMA_TILE + i) << 4);
    } else {
      As[i * ld + kb] = static_cast<uint8_t>(mfma_lp_check_code<F>(seed, blockIdx.x, i * k_total + kb));             // A[i][k]
      Bt[i * ld + kb] = static_cast<uint8_t>(mfma_lp_check_code<F>(seed, blockIdx.x, nb + kb * MFMA_TILE + i));    // B[k][i]
    }
  }
  if constexpr (mfma_lp_scaled(F)) {
    const uint32_t ns = static_cast<uint32_t>(kblocks * MFMA_TILE);
    for (uint32_t idx = t; idx < ns; idx += 256) {  // block idx / 64, row or column idx % 64
      sa[mfma_lp_scale_index(idx >> 6, idx & 63)] = mfma_lp_check_scale(seed, blockIdx.x, 2 * nb + idx);
      sb[mfma_lp_scale_index(idx >> 6, idx & 63)] = mfma_lp_check_scale(seed, blockIdx.x, 2 * nb + ns + idx);
    }
  }
  __syncthreads();
  const bool dbg = static_cast<int>(blockIdx.x) == dbg_block;
  if (dbg)
    for (uint32_t idx = t; idx < nb; idx += 256) {
      const uint32_t i = idx / k_total, k = idx - i * k_total;
      int ea = -mfma_lp_frac_bits<F>(), eb = ea;
      if constexpr (mfma_lp_scaled(F)) {
        ea += sa[mfma_lp_scale_index(k / MFMA_LP_BLOCK, i)] - MFMA_LP_SCALE_ONE;
        eb += sb[mfma_lp_scale_index(k / MFMA_LP_BLOCK, i)] - MFMA_LP_SCALE_ONE;
      }
      dbg_a[i * k_total + k] = ldexpf(static_cast<float>(mfma_lp_decode<F>(As + i * ld, k)), ea);
      dbg_b[k * MFMA_TILE + i] = ldexpf(static_cast<float>(mfma_lp_decode<F>(Bt + i * ld, k)), eb);
    }

  // round 0: the MFMA product against integer VALU arithmetic on the same LDS bytes
  const int col = mfma_tile64_col();
  // the reference's unit: the two operand units, and for the scaled formats the two smallest scales
  constexpr int UNIT_EXP = -2 * mfma_lp_frac_bits<F>() + (mfma_lp_scaled(F) ? 2 * (MFMA_LP_SCALE_MIN - MFMA_LP_SCALE_ONE) : 0);
  f32x16 want = {};
#pragma unroll 1
  for (int q = 0; q < 16; ++q) {  // one output at a time, rolled: the register count stays at four workgroups per CU
    const int row = mfma_tile64_row(q);
    const uint8_t* ar = As + row * ld;
    const uint8_t* bc = Bt + col * ld;
    long long ref = 0;
#pragma unroll 1
    for (int b = 0; b < kblocks; ++b) {
      long long dot = 0;
#pragma unroll 4
      for (int k = b * MFMA_LP_BLOCK; k < (b + 1) * MFMA_LP_BLOCK; ++k)
        dot += static_cast<long long>(mfma_lp_decode<F>(ar, k)) * mfma_lp_decode<F>(bc, k);
      int shift = 0;  // the block's two scales over the smallest: 0..4
      if constexpr (mfma_lp_scaled(F))
        shift = (sa[mfma_lp_scale_index(b, row)] - MFMA_LP_SCALE_MIN) + (sb[mfma_lp_scale_index(b, col)] - MFMA_LP_SCALE_MIN);
      ref += dot << shift;
    }
    const float w = ldexpf(static_cast<float>(ref), UNIT_EXP);  // ref has under 24 significant bits: both steps are exact
#pragma unroll
    for (int j = 0; j < 16; ++j) want[j] = j == q ? w : want[j];  // a select per register: no indexed register access
  }
  const f32x16 anchor = mfma_lp_check_product<F>(As, Bt, sa, sb);
  if (dbg) {
#pragma unroll
    for (int q = 0; q < 16; ++q) dbg_c[mfma_tile64_row(q) * MFMA_TILE + col] = anchor[q];
  }
  unsigned mine = 0;
  unsigned long long bad =
      mfma_check_compare(anchor, want, mfma_check_flip_mask(0, rounds, flips, flip_pos), 0, nrec, recs, &mine);

  // rounds 1..: re-read the operands and scales, recompute, compare bitwise with the kept round-0 accumulator
  for (int round = 1; round < rounds; ++round) {
    asm volatile("" ::: "memory");  // the operands are read from LDS again, the product is not reused
    const f32x16 c = mfma_lp_check_product<F>(As, Bt, sa, sb);
    bad += mfma_check_compare(c, anchor, mfma_check_flip_mask(round, rounds, flips, flip_pos), round, nrec,
                              recs, &mine);
  }
  if (bad) atomicAdd(errors, bad);  // one per lane that saw a mismatch: none on a healthy part
}

// ---------------------------------------------------------------------------- runners
template <int F>
inline void mfma_check_lp_launch(const MfmaCheckRun& run, int rounds, int flips, int dbg_block, float* dbg_a, float* dbg_b,
                                 float* dbg_c) {
  hipLaunchKernelGGL(mfma_check_lp_kernel<F>, dim3(run.blocks), dim3(256), 0, 0, run.seed, rounds, flips,
                     run.flip_pos.as<const uint32_t>(), run.errors.as<unsigned long long>(), run.nrec.as<unsigned>(),
                     run.recs.as<MfmaCheckRecord>(), dbg_block, dbg_a, dbg_b, dbg_c);
}

// What a format runs on: its name, its check (launch and K) and its GEMM kernel.
struct MfmaFmtOps {
  const char* name;
  MfmaCheckRun::Kernel check;
  int check_k;
  void (*gemm)(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, float*, int, int, int);
};

// throws std::invalid_argument unless fmt is in [MFMA_LP_FP8, last]
inline const MfmaFmtOps& mfma_fmt_ops(int fmt, int last = MFMA_BF16) {
  static const MfmaFmtOps ops[] = {
      {"fp8", mfma_check_lp_launch<MFMA_LP_FP8>, mfma_lp_check_kmax(MFMA_LP_FP8), mfma_gemm_lp_kernel<MFMA_LP_FP8>},
      {"mxfp8", mfma_check_lp_launch<MFMA_LP_MXFP8>, mfma_lp_check_kmax(MFMA_LP_MXFP8), mfma_gemm_lp_kernel<MFMA_LP_MXFP8>},
      {"mxfp4", mfma_check_lp_launch<MFMA_LP_MXFP4>, mfma_lp_check_kmax(MFMA_LP_MXFP4), mfma_gemm_lp_kernel<MFMA_LP_MXFP4>},
      {"bf16", mfma_check_launch_bf16, MFMA_CHECK_KMAX, nullptr}};
  if (fmt < MFMA_LP_FP8 || fmt > last) throw std::invalid_argument("unknown low-precision format");
  return ops[fmt];
}

inline const char* mfma_lp_name(int f) { return mfma_fmt_ops(f).name; }
// the format named `name` among fp8, mxfp8, mxfp4 and, with last = MFMA_BF16, bf16
inline int mfma_lp_fmt(const std::string& name, int last = MFMA_LP_MXFP4) {
  for (int f = MFMA_LP_FP8; f <= last; ++f)
    if (name == mfma_lp_name(f)) return f;
  throw std::invalid_argument("unknown low-precision dtype '" + name + "': expected fp8, mxfp8 or mxfp4");
}

// C[m x n] fp32 = A[m x k] * B[k x n] from format codes, one code per byte, row-major. fp8: e4m3fn
// codes, no scales (a_scales and b_scales empty). mxfp8 / mxfp4: e4m3fn / e2m1 codes with E8M0 scales,
// A's as [m x k/32] and B's as [k/32 x n]. Packs fp4 pairs, transposes B and A's scales for the kernel.
inline std::vector<float> mfma_gemm_lp_host(int fmt, const std::vector<uint8_t>& a, const std::vector<uint8_t>& b,
                                            const std::vector<uint8_t>& a_scales, const std::vector<uint8_t>& b_scales, int m,
                                            int n, int k, int dev) {
  const MfmaFmtOps& ops = mfma_fmt_ops(fmt, MFMA_LP_MXFP4);
  if (m <= 0 || n <= 0 || m % MFMA_TILE || n % MFMA_TILE)
    throw std::invalid_argument("M and N must be positive multiples of 64");
  const int kstep = mfma_lp_kstep(fmt);
  if (k <= 0 || k % kstep) throw std::invalid_argument("K must be a positive multiple of " + std::to_string(kstep));
  const size_t tiles = static_cast<size_t>(m / MFMA_TILE) * (n / MFMA_TILE);
  if (tiles > 0x7fffffffu) throw std::invalid_argument("too many tiles for one launch");
  if (a.size() != static_cast<size_t>(m) * k || b.size() != static_cast<size_t>(k) * n)
    throw std::invalid_argument("A must be MxK and B KxN codes");
  const size_t kblocks = mfma_lp_scaled(fmt) ? k / MFMA_LP_BLOCK : 0;
  if (a_scales.size() != kblocks * m || b_scales.size() != kblocks * n)
    throw std::invalid_argument(mfma_lp_scaled(fmt) ? "A scales must be MxK/32 and B scales K/32xN" : "fp8 takes no scales");
  if (fmt == MFMA_LP_MXFP4) {
    for (uint8_t c : a)
      if (c > 15) throw std::invalid_argument("e2m1 codes must be in [0, 15]");
    for (uint8_t c : b)
      if (c > 15) throw std::invalid_argument("e2m1 codes must be in [0, 15]");
  }
  // row images of A and of B transposed, in packed format bytes
  const size_t rb = mfma_lp_row_bytes(fmt, k);
  std::vector<uint8_t> ai(static_cast<size_t>(m) * rb), bi(static_cast<size_t>(n) * rb), sat(a_scales.size());
  if (fmt == MFMA_LP_MXFP4) {
    for (size_t i = 0; i < static_cast<size_t>(m); ++i)
      for (size_t kb = 0; kb < rb; ++kb) ai[i * rb + kb] = a[i * k + 2 * kb] | a[i * k + 2 * kb + 1] << 4;
    for (size_t j = 0; j < static_cast<size_t>(n); ++j)
      for (size_t kb = 0; kb < rb; ++kb) bi[j * rb + kb] = b[2 * kb * n + j] | b[(2 * kb + 1) * n + j] << 4;
  } else {
    ai = a;
    for (size_t j = 0; j < static_cast<size_t>(n); ++j)
      for (size_t kk = 0; kk < rb; ++kk) bi[j * rb + kk] = b[kk * n + j];
  }
  for (size_t i = 0; i < static_cast<size_t>(m); ++i)
    for (size_t kb = 0; kb < kblocks; ++kb) sat[kb * m + i] = a_scales[i * kblocks + kb];
  AK_HIP(hipSetDevice(dev));
  DevBuf da(ai), db(bi), dsa(sat), dsb(b_scales), dc(static_cast<size_t>(m) * n * sizeof(float));
  hipLaunchKernelGGL(ops.gemm, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, da.as<const uint8_t>(),
                     db.as<const uint8_t>(), dsa.as<const uint8_t>(), dsb.as<const uint8_t>(), dc.as<float>(), m, n, k);
  AK_HIP(hipGetLastError());
  return dc.download<float>();
}

// run_mfma_check on format fmt, bf16 included: rounds > 0 is one launch of exactly that many rounds,
// otherwise the run is calibrated to ~target_ms.
inline MfmaCheckResult run_mfma_check_lp(int fmt, int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu,
                                         int flips = 0) {
  const MfmaFmtOps& ops = mfma_fmt_ops(fmt);
  return mfma_check_drive(ops.check, ops.check_k, rounds, target_ms, dev, seed, flips);
}

// A and B of one workgroup decoded to fp32 with the scales applied, and its round-0 C
inline MfmaCheckTile mfma_check_lp_tile_host(int fmt, int block, uint32_t seed, int dev) {
  const MfmaFmtOps& ops = mfma_fmt_ops(fmt);
  return mfma_check_fetch_tile(ops.check, ops.check_k, block, seed, dev);
}

}  // namespace amdkube
