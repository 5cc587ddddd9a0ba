// Sparse matrix-core check: the 64x64 tile, GEMM and integrity check of mfma_check.h on the 2:4
// structured-sparsity path of CDNA4, on the run type, driver, record buffer and flip table of mfma_check.h
// and the flip mask and compare of mfma_check_wide.h. A is 2:4 sparse and travels compressed to half its
// K with one 4-bit index field per group of four k; B is dense.
//
//   sp-bf16  v_smfmac_f32_32x32x32_bf16: 8 compressed bf16 of A and 16 bf16 of B per lane, 16 index bits
//            (abid 0 / 1 picks the low / high half of the index register), 16 fp32 of C, dense K step 32
//   sp-int8  v_smfmac_i32_32x32x64_i8: 16 compressed bytes of A and 32 bytes of B per lane, 32 index
//            bits, 16 int32 of C, dense K step 64
//
// The format outside the kernel (amdkube/ops/sparse24.py): `values` is M x K/2, the kept entries of each
// group in ascending k; `meta` is M x K/32 32-bit words, group g of a row in bits 4(g mod 8).. of word
// g / 8: bits 1:0 the position (0..3) of the first kept value, bits 3:2 that of the second, the first
// strictly below the second.
//
// Lane maps as found on the MI355X with one-hot operands, one lane slot of A against every slot of B
// under each index field, and as tests/test_gpu_mfma_sparse.py holds them (lane l, r = l&31, h = l>>5;
// k counts within one instruction):
//   A      element e of the lane is compressed k 8h+e (sp-bf16) or 16h+e (sp-int8) of row r: the
//          contiguous run that was expected, the kept values of dense k 16h..16h+15 (32h..32h+31).
//   B      NOT the contiguous run 16h.. (32h..) that was first assumed: the instruction works as two
//          passes of the dense instruction of half its K. Element e of the lane is B[k][r] with
//            sp-bf16  k = 16(e>>3) + 8h + (e&7): elements 0..7 are k 8h.., elements 8..15 are k 16+8h..
//            sp-int8  k = 32(e>>4) + 16h + (e&15)
//          so lane half h of A meets B elements 8h..8h+7 (16h..16h+15) of BOTH lane halves.
//   index  field n of the lane's index bits (of the half that abid picks, for sp-bf16) goes with the
//          lane's A elements 2n and 2n+1, that is with group 4h+n (8h+n) of the row's groups of this
//          instruction: in natural order, lane half h takes 16-bit half h of the instruction's metadata
//          word (sp-bf16) or word h of its two (sp-int8). The field encoding and abid are as the ISA
//          document says.
//   C/D    the map of the dense bf16 / int8 instructions (mfma_tile64_row / mfma_tile64_col).
//
// LDS images: As[i][kc] compressed rows, Bt[j][k] dense rows of B transposed, Ms[s][i] metadata word s
// of row i, unchanged. A's traffic is half that of the dense kernel; per dense k a lane reads 1.5 operand
// bytes where the dense kernel reads 2. Bank argument (by construction; not checked with counters):
//   As, Bt  ds_read_b128, serviced in groups of 16 lanes whose rows are distinct mod 16. Every row is
//           padded by 16 bytes to an odd number of 16-byte slots: 8+1 and 16+1 slots in the check of
//           either format (64 and 128 bf16, 128 and 256 bytes), 8+1 / 16+1 (sp-bf16) and 4+1 / 8+1
//           (sp-int8) in the GEMM's slice of 128 dense k. A group's 16 rows fall on 16 distinct slots.
//   Ms      one dword per lane: the 32 lanes of a half read 32 consecutive dwords of Ms[s]. sp-bf16: both
//           halves read the same 32 addresses (a broadcast), and the words of steps s and s+1 are 64
//           dwords apart, one two-address read. sp-int8: half h reads Ms[2 ks + h], so a wave reads 64
//           consecutive dwords, each of the 64 banks once.
//
// Why the check's comparison is bitwise: operands are hashed integers, B as in the dense check of the
// element type, and every group of A has one of the six position pairs and two values of that range.
//   sp-bf16  values in [-8, 8], K/2 = 64 products: |sum| <= 64 * 64 = 2^12 < 2^24, every partial sum
//            is an fp32 number in any accumulation order.
//   sp-int8  all of -128..127, K/2 = 128 products: |sum| <= 2^14 * 128 = 2^21, exact in int32.
// The reference is integer multiply-add on the VALU from the three LDS images, B picked by the index field
// with shifts: nothing of the matrix core, its index decode included.
#pragma once

#include "mfma_check_wide.h"

namespace amdkube {

typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

constexpr int MFMA_SPARSE_GEMM_KSLICE = 128;  // dense k of one LDS slice of either GEMM
// the index fields of the six position pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), four bits each
constexpr uint32_t MFMA_SPARSE_PAIR_FIELDS = 0xED9C84u;

// dense value at position p of a group with index field f and kept values v0, v1
template <class V>
__device__ __forceinline__ V mfma_sparse_at(uint32_t f, uint32_t p, V v0, V v1) {
  return p == (f & 3u) ? v0 : p == (f >> 2) ? v1 : V(0);
}

// Σ_g Σ_s ar[2g+s] * bc[4g + pos_s] over k dense k, in int: ar a compressed row, bc a dense row of Bt,
// mrow the row's metadata words, 64 apart
template <class Elem>
__device__ __forceinline__ int mfma_sparse_reference(const Elem* ar, const Elem* bc, const uint32_t* mrow, int k) {
  int ref = 0;
#pragma unroll 1
  for (int s = 0; s < k / 32; ++s) {
    const uint32_t w = mrow[s * MFMA_TILE];
#pragma unroll 2
    for (int g8 = 0; g8 < 8; ++g8) {
      const uint32_t f = (w >> (4 * g8)) & 15u;
      const int g = 8 * s + g8;
      ref += static_cast<int>(static_cast<float>(ar[2 * g])) * static_cast<int>(static_cast<float>(bc[4 * g + (f & 3u)])) +
             static_cast<int>(static_cast<float>(ar[2 * g + 1])) * static_cast<int>(static_cast<float>(bc[4 * g + (f >> 2)]));
    }
  }
  return ref;
}

// ---------------------------------------------------------------------------- sp-bf16
struct MfmaSparseBf16 {
  typedef __bf16 Elem;
  typedef float Out;
  typedef uint32_t Bits;
  typedef f32x16 Acc;
  static constexpr int KSTEP = 32, PAD = 8, CHECK_K = 128;  // dense k; the pad is 16 bytes
  static constexpr int CHECK_WG_PER_CU = 4;

  // One K-slice of the 64x64 tile: k_steps dense steps of 32 from As (row stride lda), Bt (ldb) and Ms.
  // Two instructions per index register: the metadata words of steps 2p and 2p+1 give the register's
  // low half (abid:0) and high half (abid:1); an odd count ends on a lone abid:0.
  static __device__ __forceinline__ Acc slice(const __bf16* As, const __bf16* Bt, const uint32_t* Ms, int lda, int ldb,
                                              int k_steps, Acc acc) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
    const __bf16* ap = As + (32 * (w >> 1) + r) * lda + 8 * h;
    const __bf16* bp = Bt + (32 * (w & 1) + r) * ldb + 8 * h;
    const uint32_t* mp = Ms + 32 * (w >> 1) + r;
    const int sh = 16 * h;
    for (int p = 0; p < k_steps / 2; ++p) {
      const uint32_t m0 = mp[(2 * p) * MFMA_TILE], m1 = mp[(2 * p + 1) * MFMA_TILE];
      const int idx = static_cast<int>(((m0 >> sh) & 0xffffu) | ((m1 >> sh) << 16));  // half h of either word
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap + 32 * p), a1 = *reinterpret_cast<const bf16x8*>(ap + 32 * p + 16);
      acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a0, b_of_step(bp + 64 * p), acc, idx, 0, 0);
      acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a1, b_of_step(bp + 64 * p + 32), acc, idx, 0, 1);
    }
    if (k_steps & 1) {
      const int s = k_steps - 1;
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(ap + 16 * s);
      acc = __builtin_amdgcn_smfmac_f32_32x32x32_bf16(a0, b_of_step(bp + 32 * s), acc, static_cast<int>(mp[s * MFMA_TILE] >> sh), 0, 0);
    }
    return acc;
  }
  // the lane's 16 B values of one step: k 8h..8h+7 and 16+8h..16+8h+7, p at the first
  static __device__ __forceinline__ bf16x16 b_of_step(const __bf16* p) {
    return __builtin_shufflevector(*reinterpret_cast<const bf16x8*>(p), *reinterpret_cast<const bf16x8*>(p + 16), 0, 1, 2, 3, 4, 5, 6,
                                   7, 8, 9, 10, 11, 12, 13, 14, 15);
  }
  static __device__ __forceinline__ int row(int e) { return mfma_tile64_row(e); }
  static __device__ __forceinline__ int col(int) { return mfma_tile64_col(); }
  static __device__ __forceinline__ int elem_of(uint32_t row, uint32_t col) { return MfmaWideInt8::elem_of(row, col); }
  static __device__ __forceinline__ Out value(const Acc& a, int e) { return a[e]; }
  static __device__ __forceinline__ Bits bits(const Acc& a, int e) { return __float_as_uint(a[e]); }
  static __device__ __forceinline__ void flip(Acc& a, uint32_t mask) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = __uint_as_float(__float_as_uint(a[e]) ^ ((mask >> e) & 1u));
  }
  static __device__ __forceinline__ void record_words(Bits g, Bits w, uint32_t* got, uint32_t* want) {
    *got = g;
    *want = w;
  }
  // operand of the check: an integer in [-8, 8]
  static __device__ __forceinline__ Elem check_value(uint32_t seed, uint32_t block, uint32_t index) {
    return static_cast<__bf16>(mfma_check_value(seed, block, index));
  }
  static __device__ __forceinline__ Bits reference(const Elem* ar, const Elem* bc, const uint32_t* mrow) {
    return __float_as_uint(static_cast<float>(mfma_sparse_reference(ar, bc, mrow, CHECK_K)));
  }
};

// ---------------------------------------------------------------------------- sp-int8
// the accumulators, their place in the tile, the compared bits and the hashed operand are the dense int8 ones
struct MfmaSparseInt8 : MfmaWideInt8 {
  static constexpr int KSTEP = 64, PAD = 16, CHECK_K = 256;

  // k_steps dense steps of 64; lane half h takes metadata word h of the step's two as its index register
  static __device__ __forceinline__ Acc slice(const int8_t* As, const int8_t* Bt, const uint32_t* Ms, int lda, int ldb,
                                              int k_steps, Acc acc) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
    const int8_t* ap = As + (32 * (w >> 1) + r) * lda + 16 * h;
    const int8_t* bp = Bt + (32 * (w & 1) + r) * ldb + 16 * h;
    const uint32_t* mp = Ms + h * MFMA_TILE + 32 * (w >> 1) + r;
    for (int ks = 0; ks < k_steps; ++ks) {
      const int idx = static_cast<int>(mp[2 * ks * MFMA_TILE]);
      const lp_v4i a = *reinterpret_cast<const lp_v4i*>(ap + 32 * ks);
      const lp_v4i b0 = *reinterpret_cast<const lp_v4i*>(bp + 64 * ks), b1 = *reinterpret_cast<const lp_v4i*>(bp + 64 * ks + 32);
      acc = __builtin_amdgcn_smfmac_i32_32x32x64_i8(a, __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7), acc, idx, 0, 0);
    }
    return acc;
  }
  static __device__ __forceinline__ Bits reference(const Elem* ar, const Elem* bc, const uint32_t* mrow) {
    return static_cast<Bits>(mfma_sparse_reference(ar, bc, mrow, CHECK_K));
  }
};

// ---------------------------------------------------------------------------- GEMM on caller data
// the metadata words of this slice: word s of row i to Ms[s][i]; 4 x 64 words, one per thread
__device__ __forceinline__ void mfma_sparse_load_meta(uint32_t* Ms, const uint32_t* __restrict__ meta, size_t m0, int K, int k0,
                                                      int kk) {
  const int s = threadIdx.x >> 6, i = threadIdx.x & 63;
  if (32 * s < kk) Ms[s * MFMA_TILE + i] = meta[(m0 + i) * (K / 32) + k0 / 32 + s];
}

// C[MxN] fp32 = A * B, A 2:4 sparse as values [M x K/2] bf16 and meta [M x K/32] words, B [K x N] bf16
// row-major; one workgroup per 64x64 tile of C, M and N multiples of 64, K a multiple of 32 (checked by
// mfma_gemm_sparse_host). A ragged last slice runs (K mod 128) / 32 steps on the part of the images that
// was filled.
__global__ __launch_bounds__(256) void mfma_gemm_sparse_bf16_kernel(const __bf16* __restrict__ V, const uint32_t* __restrict__ meta,
                                                                    const __bf16* __restrict__ B, float* __restrict__ C, int M,
                                                                    int N, int K) {
  typedef MfmaSparseBf16 T;
  constexpr int KS = MFMA_SPARSE_GEMM_KSLICE, LDA = KS / 2 + T::PAD, LDB = KS + T::PAD;
  __shared__ __attribute__((aligned(16))) __bf16 As[MFMA_TILE * LDA];  // 9 KiB
  __shared__ __attribute__((aligned(16))) __bf16 Bt[MFMA_TILE * LDB];  // 17 KiB
  __shared__ uint32_t Ms[(KS / 32) * MFMA_TILE];                       // 1 KiB
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  T::Acc acc = mfma_wide_zero<T>();
  for (int k0 = 0; k0 < K; k0 += KS) {
    const int kk = K - k0 < KS ? K - k0 : KS;  // a multiple of 32
    // compressed A: 64 rows x 8 chunks of 8 values, copied as they lie
    for (int c = t; c < MFMA_TILE * (KS / 16); c += 256) {
      const int row = c >> 3, kc = (c & 7) * 8;
      if (kc < kk / 2)
        *reinterpret_cast<bf16x8*>(As + row * LDA + kc) = *reinterpret_cast<const bf16x8*>(V + (m0 + row) * (K / 2) + k0 / 2 + kc);
    }
    // B slice, transposed: wave w takes k rows 32w..32w+31, lane l column l
    const int kb = 32 * w;
    if (kb < kk) {
#pragma unroll
      for (int c = 0; c < 32; c += 8) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = B[static_cast<size_t>(k0 + kb + c + j) * N + n0 + l];
        *reinterpret_cast<bf16x8*>(Bt + l * LDB + kb + c) = v;
      }
    }
    mfma_sparse_load_meta(Ms, meta, m0, K, k0, kk);
    __syncthreads();
    acc = T::slice(As, Bt, Ms, LDA, LDB, kk / T::KSTEP, acc);
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) C[(m0 + T::row(e)) * N + n0 + T::col(e)] = T::value(acc, e);
}

// C[MxN] int32 = A * B on caller bytes: A as values [M x K/2] and meta [M x K/32], Bt the N x K image of
// B transposed (mfma_gemm_sparse_host transposes), int8. M and N multiples of 64, K a multiple of 64.
__global__ __launch_bounds__(256) void mfma_gemm_sparse_int8_kernel(const int8_t* __restrict__ V, const uint32_t* __restrict__ meta,
                                                                    const int8_t* __restrict__ Bt, int* __restrict__ C, int M,
                                                                    int N, int K) {
  typedef MfmaSparseInt8 T;
  constexpr int KS = MFMA_SPARSE_GEMM_KSLICE, LDA = KS / 2 + T::PAD, LDB = KS + T::PAD;  // 80 and 144 B: 5 and 9 slots
  __shared__ __attribute__((aligned(16))) int8_t As[MFMA_TILE * LDA];
  __shared__ __attribute__((aligned(16))) int8_t Bs[MFMA_TILE * LDB];
  __shared__ uint32_t Ms[(KS / 32) * MFMA_TILE];
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x;
  T::Acc acc = mfma_wide_zero<T>();
  for (int k0 = 0; k0 < K; k0 += KS) {
    const int kk = K - k0 < KS ? K - k0 : KS;  // a multiple of 64
    for (int c = t; c < MFMA_TILE * (KS / 16); c += 256) {
      const int row = c >> 3, off = (c & 7) * 16;
      if (off < kk / 2)  // the compressed row is the first half of the chunks
        *reinterpret_cast<uint4*>(As + row * LDA + off) = *reinterpret_cast<const uint4*>(V + (m0 + row) * (K / 2) + k0 / 2 + off);
      if (off < kk)
        *reinterpret_cast<uint4*>(Bs + row * LDB + off) = *reinterpret_cast<const uint4*>(Bt + (n0 + row) * K + k0 + off);
    }
    mfma_sparse_load_meta(Ms, meta, m0, K, k0, kk);
    __syncthreads();
    acc = T::slice(As, Bs, Ms, LDA, LDB, kk / T::KSTEP, acc);
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) C[(m0 + T::row(e)) * N + n0 + T::col(e)] = T::value(acc, e);
}

// ---------------------------------------------------------------------------- the check
// mfma_check_wide_kernel with the third image: the check of mfma_check_kernel on sparse format T at dense
// K = T::CHECK_K. rounds >= 1; flip_pos holds MFMA_CHECK_MAX_FLIPS entries. Hash indices of a workgroup:
// compressed A value (i, kc) at i K/2 + kc, the position pair of group (i, g) at 64 K/2 + i K/4 + g, and
// B[k][j] at 64 K + 64 k + j, which is the B of the dense check of the same K.
// dbg_block >= 0: that workgroup also stores its A expanded to dense [64 x K], B[K x 64] and round-0
// C[64 x 64] as doubles (tests only).
template <class T>
__global__ __launch_bounds__(256, T::CHECK_WG_PER_CU) void mfma_check_sparse_kernel(
    uint32_t seed, int rounds, int flips, const uint32_t* __restrict__ flip_pos, unsigned long long* __restrict__ errors,
    unsigned* __restrict__ nrec, MfmaCheckRecord* __restrict__ recs, int dbg_block, double* __restrict__ dbg_a,
    double* __restrict__ dbg_b, double* __restrict__ dbg_c) {
  typedef typename T::Elem Elem;
  typedef typename T::Acc Acc;
  constexpr int K = T::CHECK_K, KC = K / 2, LDA = KC + T::PAD, LDB = K + T::PAD, STEPS = K / T::KSTEP, WORDS = K / 32;
  __shared__ __attribute__((aligned(16))) Elem As[MFMA_TILE * LDA];  // 9 + 17 + 1 (sp-int8: 2) KiB
  __shared__ __attribute__((aligned(16))) Elem Bt[MFMA_TILE * LDB];
  __shared__ uint32_t Ms[WORDS * MFMA_TILE];
  // uniform: never index past the flip table, never loop on a non-positive stride
  if (rounds < 1 || flips < 0 || flips > MFMA_CHECK_MAX_FLIPS) return;
  const int t = threadIdx.x;
  constexpr uint32_t na = MFMA_TILE * KC, nb = MFMA_TILE * K;
  for (uint32_t idx = t; idx < nb; idx += 256) {
    const uint32_t i = idx / K, k = idx - i * K;
    if (idx < na) As[(idx / KC) * LDA + idx % KC] = T::check_value(seed, blockIdx.x, idx);  // compressed A[idx / KC][idx % KC]
    Bt[i * LDB + k] = T::check_value(seed, blockIdx.x, nb + k * MFMA_TILE + i);              // B[k][i]
  }
  for (uint32_t idx = t; idx < WORDS * MFMA_TILE; idx += 256) {
    const uint32_t s = idx / MFMA_TILE, i = idx % MFMA_TILE;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t g8 = 0; g8 < 8; ++g8) {
      const uint32_t pair = mix32(seed, blockIdx.x, na + i * (K / 4) + 8 * s + g8) % 6u;
      word |= ((MFMA_SPARSE_PAIR_FIELDS >> (4 * pair)) & 15u) << (4 * g8);
    }
    Ms[idx] = word;
  }
  __syncthreads();
  const bool dbg = static_cast<int>(blockIdx.x) == dbg_block;
  if (dbg)
    for (uint32_t idx = t; idx < nb; idx += 256) {
      const uint32_t i = idx / K, k = idx - i * K, g = k >> 2;
      const uint32_t f = (Ms[(g >> 3) * MFMA_TILE + i] >> (4 * (g & 7))) & 15u;
      dbg_a[i * K + k] = mfma_sparse_at(f, k & 3u, static_cast<double>(As[i * LDA + 2 * g]), static_cast<double>(As[i * LDA + 2 * g + 1]));
      dbg_b[k * MFMA_TILE + i] = static_cast<double>(Bt[i * LDB + k]);
    }

  // round 0: the sparse product against integer VALU arithmetic on the same LDS images
  const Acc anchor = T::slice(As, Bt, Ms, LDA, LDB, STEPS, mfma_wide_zero<T>());
  if (dbg) {
#pragma unroll
    for (int e = 0; e < 16; ++e) dbg_c[T::row(e) * MFMA_TILE + T::col(e)] = static_cast<double>(T::value(anchor, e));
  }
  unsigned mine = 0;
  unsigned long long bad = mfma_wide_compare<T, 1>(
      anchor, [&](int e) { return T::reference(As + T::row(e) * LDA, Bt + T::col(e) * LDB, Ms + T::row(e)); },
      mfma_wide_flip_mask<T>(0, rounds, flips, flip_pos), 0, nrec, recs, &mine);

  // rounds 1..: re-read operands and metadata, recompute, compare bitwise with the kept round-0 accumulators
  for (int round = 1; round < rounds; ++round) {
    asm volatile("" ::: "memory");  // the images are read from LDS again, the product is not reused
    const Acc c = T::slice(As, Bt, Ms, LDA, LDB, STEPS, mfma_wide_zero<T>());
    bad += mfma_wide_compare<T, 16>(c, [&](int e) { return mfma_wide_pick<T>(anchor, e); },
                                    mfma_wide_flip_mask<T>(round, rounds, flips, flip_pos), round, nrec, recs, &mine);
  }
  if (bad) atomicAdd(errors, bad);  // one per lane that saw a mismatch: none on a healthy part
}

// ---------------------------------------------------------------------------- runners
template <class T>
inline void mfma_check_sparse_launch(const MfmaCheckRun& run, int rounds, int flips, int dbg_block, void* dbg_a, void* dbg_b,
                                     void* dbg_c) {
  hipLaunchKernelGGL(mfma_check_sparse_kernel<T>, dim3(run.blocks), dim3(256), 0, 0, run.seed, rounds, flips,
                     run.flip_pos.as<const uint32_t>(), run.errors.as<unsigned long long>(), run.nrec.as<unsigned>(),
                     run.recs.as<MfmaCheckRecord>(), dbg_block, static_cast<double*>(dbg_a), static_cast<double*>(dbg_b),
                     static_cast<double*>(dbg_c));
}

inline bool mfma_fmt_is_sparse(int fmt) { return fmt == MFMA_SPARSE_BF16 || fmt == MFMA_SPARSE_INT8; }

// mfma_fmt_ops over every format of the check: the wide and the sparse ones have no GEMM in that table.
// check_k of a sparse format is its dense K, so a rate counts the dense-equivalent 2 * 64 * 64 * K.
inline const MfmaFmtOps& mfma_check_fmt_ops(int fmt) {
  static const MfmaFmtOps more[] = {{"fp64", mfma_check_wide_launch<MfmaWideFp64>, MfmaWideFp64::CHECK_K, nullptr},
                                    {"int8", mfma_check_wide_launch<MfmaWideInt8>, MfmaWideInt8::CHECK_K, nullptr},
                                    {"sp-bf16", mfma_check_sparse_launch<MfmaSparseBf16>, MfmaSparseBf16::CHECK_K, nullptr},
                                    {"sp-int8", mfma_check_sparse_launch<MfmaSparseInt8>, MfmaSparseInt8::CHECK_K, nullptr}};
  return mfma_fmt_is_wide(fmt) || mfma_fmt_is_sparse(fmt) ? more[fmt - MFMA_WIDE_FP64] : mfma_fmt_ops(fmt);
}

// fp64, int8, sp-bf16 or sp-int8, else what mfma_lp_fmt(name, last) says
inline int mfma_check_fmt(const std::string& name, int last = MFMA_LP_MXFP4) {
  for (int f = MFMA_WIDE_FP64; f <= MFMA_SPARSE_INT8; ++f)
    if (name == mfma_check_fmt_ops(f).name) return f;
  return mfma_lp_fmt(name, last);
}

// run_mfma_check_lp over every format of the check
inline MfmaCheckResult run_mfma_check_fmt(int fmt, int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu,
                                          int flips = 0) {
  const MfmaFmtOps& ops = mfma_check_fmt_ops(fmt);
  return mfma_check_drive(ops.check, ops.check_k, rounds, target_ms, dev, seed, flips);
}

// A (expanded to dense for the sparse formats), B and the round-0 C of one workgroup of a wide or sparse check, as doubles
inline MfmaCheckTileOf<double> mfma_check_wide_tile_host(int fmt, int block, uint32_t seed, int dev) {
  if (!mfma_fmt_is_wide(fmt) && !mfma_fmt_is_sparse(fmt)) throw std::invalid_argument("not a wide or sparse format");
  const MfmaFmtOps& ops = mfma_check_fmt_ops(fmt);
  return mfma_check_fetch_tile<double>(ops.check, ops.check_k, block, seed, dev);
}

// C[m x n] = A * B with A 2:4 sparse: `values` holds the m x k/2 kept entries and `b` the k x n dense B,
// row-major, as the raw bytes of bf16 (sp-bf16) or int8 (sp-int8) elements; `meta` is m x k/32 words.
// Returns the words of C, fp32 or int32. Transposes B for sp-int8.
inline std::vector<uint32_t> mfma_gemm_sparse_host(int fmt, const std::vector<uint8_t>& values, const std::vector<uint32_t>& meta,
                                                   const std::vector<uint8_t>& b, int m, int n, int k, int dev) {
  if (!mfma_fmt_is_sparse(fmt)) throw std::invalid_argument("not a sparse format");
  const bool i8 = fmt == MFMA_SPARSE_INT8;
  const size_t es = i8 ? 1 : 2;
  const size_t tiles = mfma_wide_tiles(m, n, k, i8 ? MfmaSparseInt8::KSTEP : MfmaSparseBf16::KSTEP);
  if (values.size() != static_cast<size_t>(m) * (k / 2) * es || meta.size() != static_cast<size_t>(m) * (k / 32) ||
      b.size() != static_cast<size_t>(k) * n * es)
    throw std::invalid_argument("values must be MxK/2, meta MxK/32 words and B KxN");
  for (uint32_t w : meta)
    for (int g = 0; g < 8; ++g) {
      const uint32_t f = (w >> (4 * g)) & 15u;
      if ((f & 3u) >= (f >> 2)) throw std::invalid_argument("an index field must have its first position below its second");
    }
  AK_HIP(hipSetDevice(dev));
  DevBuf dv(values), dm(meta), dc(static_cast<size_t>(m) * n * 4);
  dc.fill(0xff);  // a value the kernel never wrote cannot pass
  if (i8) {
    std::vector<uint8_t> bt(b.size());
    for (size_t j = 0; j < static_cast<size_t>(n); ++j)
      for (size_t kk = 0; kk < static_cast<size_t>(k); ++kk) bt[j * k + kk] = b[kk * n + j];
    DevBuf db(bt);
    hipLaunchKernelGGL(mfma_gemm_sparse_int8_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, dv.as<const int8_t>(),
                       dm.as<const uint32_t>(), db.as<const int8_t>(), dc.as<int>(), m, n, k);
    AK_HIP(hipGetLastError());
    return dc.download<uint32_t>();
  }
  DevBuf db(b);
  hipLaunchKernelGGL(mfma_gemm_sparse_bf16_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, dv.as<const __bf16>(),
                     dm.as<const uint32_t>(), db.as<const __bf16>(), dc.as<float>(), m, n, k);
  AK_HIP(hipGetLastError());
  return dc.download<uint32_t>();
}

}  // namespace amdkube
