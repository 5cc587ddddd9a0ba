// Wide matrix-core check: the 64x64 tile, GEMM and integrity check of mfma_check.h on the two matrix
// datapaths of CDNA4 that do not accumulate in fp32, on the run type, driver, record buffer and flip
// table of mfma_check.h. The accumulators, the compare and the tile dump are typed per format here.
//
//   fp64   v_mfma_f64_16x16x4_f64: one double per lane for A and for B, four doubles of C, K step 4
//   int8   v_mfma_i32_32x32x32_i8: 16 bytes per lane for A and for B, 16 int32 of C, K step 32
//
// Lane maps, as the kernels use them and as the one-hot and exact-GEMM tests of
// tests/test_gpu_mfma_wide.py check them on the part:
//   fp64   lane l, i = l&15, kq = l>>4 feeds A[i][kq] and B[kq][i]; accumulator register q is
//          C[4 q + kq][i]: a lane's four rows are four apart, not adjacent. (With C[4 kq + q][i], as first
//          written, the one-hot test got the rows of each 16x16 block transposed as a 4x4 grid on the
//          part: right only where q = kq.) A wave's 32x32 quadrant is 2x2 such blocks: block (bi, bj) multiplies the
//          A register of rows 16 bi.. with the B register of columns 16 bj.., so each of the two A and
//          two B registers of a K step feeds two of its four MFMAs.
//   int8   lane l, r = l&31, h = l>>5: byte j of the 128-bit operand is A[r][16h+j] and B[16h+j][r];
//          the C/D map is the bf16 one (mfma_tile64_row / mfma_tile64_col). The part agreed with both.
//
// LDS images are rows As[i][k] and Bt[j][k], as in the other formats.
//   fp64   rows of doubles, K slice 32 and a pad of 2: ld = 34. A ds_read_b64 is serviced per 32-lane
//          half; such a half reads 16 consecutive rows at two adjacent kq. With ld = 2 (mod 32) its
//          8-byte slot is 2 row + kq + const (mod 32): 32 distinct slots of the 256-byte bank row, so
//          the read is conflict-free.
//   int8   rows of bytes with a pad of 16: the stride is an odd number of 16-byte slots (row bytes are
//          a multiple of 32), the argument mfma_lp_pad makes for ds_read_b128.
//
// Why the check's comparison is bitwise:
//   fp64   operands are hashed integers with |v| <= 2^23, so nearly all of the 53-bit multiplier is in
//          use. A product is at most 2^46 and a sum of 32 at most 2^51 < 2^53: every partial sum is an
//          fp64 number in any accumulation order. The reference is long long multiply-add on the VALU.
//   int8   operands are hashed over all of -128..127. |sum| <= 2^14 * 256 = 2^22: exact in int32. The
//          reference is plain int multiply-add on the VALU from the LDS bytes.
#pragma once

#include "mfma_check_lp.h"

namespace amdkube {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------- fp64
// What a format is to the check kernel: its LDS element, its accumulators as 16 values per lane
// (element e, a compile-time index wherever it is used), their place in the tile, the bits that are
// compared, the hashed operand and the exact reference.
struct MfmaWideFp64 {
  typedef double Elem;    // LDS and caller operands
  typedef double Out;     // C
  typedef uint64_t Bits;  // what the compare sees of one value
  struct Acc {
    f64x4 b[4];  // block (bi, bj) of the quadrant at b[2 bi + bj]: element e is b[e >> 2][e & 3]
  };
  static constexpr int KSTEP = 4, KSLICE = 32, PAD = 2, CHECK_K = 32;
  static constexpr int CHECK_WG_PER_CU = 4;
  static constexpr int VALUE_MAX = 1 << 23;  // |operand| of the check

  // One K-slice of the 64x64 tile, operands in LDS with row stride ld doubles: k_steps steps of 4.
  static __device__ __forceinline__ Acc slice(const double* As, const double* Bt, int ld, int k_steps, Acc acc) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, i = l & 15, kq = l >> 4;
    const double* ap = As + (32 * (w >> 1) + i) * ld + kq;
    const double* bp = Bt + (32 * (w & 1) + i) * ld + kq;
    for (int ks = 0; ks < k_steps; ++ks) {
      const double a0 = ap[4 * ks], a1 = ap[16 * ld + 4 * ks];
      const double b0 = bp[4 * ks], b1 = bp[16 * ld + 4 * ks];
      acc.b[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc.b[0], 0, 0, 0);
      acc.b[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc.b[1], 0, 0, 0);
      acc.b[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc.b[2], 0, 0, 0);
      acc.b[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc.b[3], 0, 0, 0);
    }
    return acc;
  }
  // tile row and column of element e of this lane
  static __device__ __forceinline__ int row(int e) {
    const int w = threadIdx.x >> 6, kq = (threadIdx.x >> 4) & 3;
    return 32 * (w >> 1) + 16 * (e >> 3) + 4 * (e & 3) + kq;
  }
  static __device__ __forceinline__ int col(int e) {
    return 32 * ((threadIdx.x >> 6) & 1) + 16 * ((e >> 2) & 1) + (threadIdx.x & 15);
  }
  // the element of this lane that is tile position (row, col), or -1
  static __device__ __forceinline__ int elem_of(uint32_t row, uint32_t col) {
    const uint32_t w = threadIdx.x >> 6, kq = (threadIdx.x >> 4) & 3, i = threadIdx.x & 15;
    if ((row >> 5) != (w >> 1) || (col >> 5) != (w & 1) || (col & 15) != i || (row & 3) != kq) return -1;
    return static_cast<int>(8 * ((row >> 4) & 1) + 4 * ((col >> 4) & 1) + ((row >> 2) & 3));
  }
  static __device__ __forceinline__ Out value(const Acc& a, int e) { return a.b[e >> 2][e & 3]; }
  static __device__ __forceinline__ Bits bits(const Acc& a, int e) {
    return static_cast<Bits>(__double_as_longlong(a.b[e >> 2][e & 3]));
  }
  // XOR bit 0 of the low word of the elements in `mask`
  static __device__ __forceinline__ void flip(Acc& a, uint32_t mask) {
#pragma unroll
    for (int e = 0; e < 16; ++e)
      a.b[e >> 2][e & 3] = __longlong_as_double(__double_as_longlong(a.b[e >> 2][e & 3]) ^ static_cast<long long>((mask >> e) & 1u));
  }
  // the 32-bit half of a mismatching pair that a record shows: the low one if it differs, as cu_check.h does
  static __device__ __forceinline__ void record_words(Bits g, Bits w, uint32_t* got, uint32_t* want) {
    const int shift = static_cast<uint32_t>(g) != static_cast<uint32_t>(w) ? 0 : 32;
    *got = static_cast<uint32_t>(g >> shift);
    *want = static_cast<uint32_t>(w >> shift);
  }
  // operand of the check: an integer in [-2^23, 2^23]
  static __device__ __forceinline__ Elem check_value(uint32_t seed, uint32_t block, uint32_t index) {
    return static_cast<double>(static_cast<int>(mix32(seed, block, index) % (2u * VALUE_MAX + 1u)) - VALUE_MAX);
  }
  // bits of the exact dot product of two LDS rows: 64-bit integer arithmetic, |sum| < 2^53
  static __device__ __forceinline__ Bits reference(const Elem* ar, const Elem* bc) {
    long long ref = 0;
#pragma unroll 4
    for (int k = 0; k < CHECK_K; ++k) ref += static_cast<long long>(static_cast<int>(ar[k])) * static_cast<int>(bc[k]);
    return static_cast<Bits>(__double_as_longlong(static_cast<double>(ref)));
  }
};

// ---------------------------------------------------------------------------- int8
struct MfmaWideInt8 {
  typedef int8_t Elem;
  typedef int Out;
  typedef uint32_t Bits;
  typedef i32x16 Acc;
  static constexpr int KSTEP = 32, KSLICE = 128, PAD = 16, CHECK_K = 256;
  static constexpr int CHECK_WG_PER_CU = 4;

  // One K-slice of the 64x64 tile, operands in LDS with row stride ld bytes (a multiple of 16): k_steps steps of 32.
  static __device__ __forceinline__ Acc slice(const int8_t* As, const int8_t* Bt, int ld, int k_steps, Acc acc) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 31, h = l >> 5;
    const int8_t* ap = As + (32 * (w >> 1) + r) * ld + 16 * h;
    const int8_t* bp = Bt + (32 * (w & 1) + r) * ld + 16 * h;
    for (int ks = 0; ks < k_steps; ++ks) {
      const lp_v4i a = *reinterpret_cast<const lp_v4i*>(ap + 32 * ks);
      const lp_v4i b = *reinterpret_cast<const lp_v4i*>(bp + 32 * ks);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
    }
    return acc;
  }
  static __device__ __forceinline__ int row(int e) { return mfma_tile64_row(e); }
  static __device__ __forceinline__ int col(int) { return mfma_tile64_col(); }
  static __device__ __forceinline__ int elem_of(uint32_t row, uint32_t col) {
    const uint32_t w = threadIdx.x >> 6, h = (threadIdx.x >> 5) & 1;
    if (col != static_cast<uint32_t>(mfma_tile64_col()) || (row >> 5) != (w >> 1) || ((row >> 2) & 1) != h) return -1;
    return static_cast<int>((row & 3) + 4 * ((row & 31) >> 3));
  }
  static __device__ __forceinline__ Out value(const Acc& a, int e) { return a[e]; }
  static __device__ __forceinline__ Bits bits(const Acc& a, int e) { return static_cast<Bits>(a[e]); }
  static __device__ __forceinline__ void flip(Acc& a, uint32_t mask) {
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] ^= static_cast<int>((mask >> e) & 1u);
  }
  static __device__ __forceinline__ void record_words(Bits g, Bits w, uint32_t* got, uint32_t* want) {
    *got = g;
    *want = w;
  }
  // operand of the check: all of -128..127
  static __device__ __forceinline__ Elem check_value(uint32_t seed, uint32_t block, uint32_t index) {
    return static_cast<int8_t>(mix32(seed, block, index) & 0xffu);
  }
  // the exact dot product of two LDS rows, a byte at a time: nothing of the unit under test
  static __device__ __forceinline__ Bits reference(const Elem* ar, const Elem* bc) {
    int ref = 0;
#pragma unroll 4
    for (int k = 0; k < CHECK_K; ++k) ref += static_cast<int>(ar[k]) * static_cast<int>(bc[k]);
    return static_cast<Bits>(ref);
  }
};

template <class T>
__device__ __forceinline__ typename T::Acc mfma_wide_zero() {
  typename T::Acc z = {};
  return z;
}

// ---------------------------------------------------------------------------- GEMM on caller data
// C[MxN] fp64 = A[MxK] * B[KxN], all row-major fp64; one workgroup per 64x64 tile of C, M and N
// multiples of 64, K a multiple of 4 (checked by mfma_gemm_fp64_host). A ragged last slice runs
// (K mod 32) / 4 steps on the part of the images that was filled.
__global__ __launch_bounds__(256) void mfma_gemm_fp64_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                             double* __restrict__ C, int M, int N, int K) {
  typedef MfmaWideFp64 T;
  constexpr int LD = T::KSLICE + T::PAD;
  __shared__ __attribute__((aligned(16))) double As[MFMA_TILE * LD];  // 2 x 64 x 34 x 8 B = 34 KiB
  __shared__ __attribute__((aligned(16))) double Bt[MFMA_TILE * LD];
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  T::Acc acc = mfma_wide_zero<T>();
  for (int k0 = 0; k0 < K; k0 += T::KSLICE) {
    const int kk = K - k0 < T::KSLICE ? K - k0 : T::KSLICE;  // a multiple of 4
    // A slice: 64 rows x 16 pairs of doubles, copied as they lie (K is even: every pair is 16-byte aligned)
    for (int c = t; c < MFMA_TILE * (T::KSLICE / 2); c += 256) {
      const int row = c >> 4, kc = (c & 15) * 2;
      if (kc < kk)
        *reinterpret_cast<f64x2*>(As + row * LD + kc) = *reinterpret_cast<const f64x2*>(A + (m0 + row) * K + k0 + kc);
    }
    // B slice, transposed: wave w takes k rows 8w..8w+7, lane l column l (512 contiguous bytes per row)
    const int kb = 8 * w;
#pragma unroll
    for (int j = 0; j < 8; j += 2)
      if (kb + j < kk) {  // kk is even: the pair is inside or outside as one
        const f64x2 v = {B[static_cast<size_t>(k0 + kb + j) * N + n0 + l], B[static_cast<size_t>(k0 + kb + j + 1) * N + n0 + l]};
        *reinterpret_cast<f64x2*>(Bt + l * LD + kb + j) = v;
      }
    __syncthreads();
    acc = T::slice(As, Bt, LD, kk / T::KSTEP, acc);
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) C[(m0 + T::row(e)) * N + n0 + T::col(e)] = T::value(acc, e);
}

// C[MxN] int32 = A * B on caller bytes: A is the M x K image of A and Bt the N x K image of B
// transposed (mfma_gemm_int8_host transposes), int8. M and N multiples of 64, K a multiple of 32.
__global__ __launch_bounds__(256) void mfma_gemm_int8_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ Bt,
                                                             int* __restrict__ C, int M, int N, int K) {
  typedef MfmaWideInt8 T;
  constexpr int LD = T::KSLICE + T::PAD;  // 144 B: nine 16-byte slots
  __shared__ __attribute__((aligned(16))) int8_t As[MFMA_TILE * LD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[MFMA_TILE * LD];
  const int tiles_n = N / MFMA_TILE;
  const size_t m0 = static_cast<size_t>(blockIdx.x / tiles_n) * MFMA_TILE;
  const size_t n0 = static_cast<size_t>(blockIdx.x % tiles_n) * MFMA_TILE;
  if (m0 >= static_cast<size_t>(M)) return;  // whole workgroup: the grid is one block per tile
  const int t = threadIdx.x;
  T::Acc acc = mfma_wide_zero<T>();
  for (int k0 = 0; k0 < K; k0 += T::KSLICE) {
    const int kk = K - k0 < T::KSLICE ? K - k0 : T::KSLICE;  // a multiple of 32
    for (int c = t; c < MFMA_TILE * (T::KSLICE / 16); c += 256) {
      const int row = c >> 3, off = (c & 7) * 16;
      if (off < kk) {
        *reinterpret_cast<uint4*>(As + row * LD + off) = *reinterpret_cast<const uint4*>(A + (m0 + row) * K + k0 + off);
        *reinterpret_cast<uint4*>(Bs + row * LD + off) = *reinterpret_cast<const uint4*>(Bt + (n0 + row) * K + k0 + off);
      }
    }
    __syncthreads();
    acc = T::slice(As, Bs, LD, kk / T::KSTEP, acc);
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) C[(m0 + T::row(e)) * N + n0 + T::col(e)] = T::value(acc, e);
}

// ---------------------------------------------------------------------------- the check
// mfma_check_flip_mask with the row / column map of T: the self-test flips of round `round` that land
// on this lane, as a mask over its 16 elements.
template <class T>
__device__ __forceinline__ uint32_t mfma_wide_flip_mask(int round, int rounds, int flips, const uint32_t* flip_pos) {
  uint32_t m = 0;
  for (long long i = round; i < flips; i += rounds) {
    const uint32_t p = flip_pos[i];
    const int e = (p >> 12) == blockIdx.x ? T::elem_of((p >> 6) & 63, p & 63) : -1;
    if (e >= 0) m |= 1u << e;
  }
  return m;
}

// bits of element e of `a`, e known at run time only: a select per register, no indexed register access
template <class T>
__device__ __forceinline__ typename T::Bits mfma_wide_pick(const typename T::Acc& a, int e) {
  typename T::Bits r = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) r = j == e ? T::bits(a, j) : r;
  return r;
}

// mfma_check_compare on T's accumulators: want(e) gives the bits element e must have. flip_mask XORs
// bit 0 (of the low word, for fp64) of `got`, which is the compared copy only. One branch on the healthy
// path; `want` is evaluated again for the records, so a reference that is costly to compute is kept in
// no register, and the flips are made in place, so the records need no second copy of `got` either.
// UNROLL is 16 where want(e) is a register (later rounds) and 1 where it is a loop over K (round 0):
// sixteen interleaved copies of that loop cost more registers than four workgroups per CU leave.
template <class T, int UNROLL, class Want>
__device__ __forceinline__ unsigned mfma_wide_compare(typename T::Acc got, Want&& want, uint32_t flip_mask, int round,
                                                      unsigned* nrec, MfmaCheckRecord* recs, unsigned* mine) {
  typedef typename T::Bits Bits;
  T::flip(got, flip_mask);
  Bits diff = 0;
#pragma unroll UNROLL
  for (int e = 0; e < 16; ++e) diff |= mfma_wide_pick<T>(got, e) ^ want(e);
  if (diff == 0) return 0;
  unsigned bad = 0;
#pragma unroll 1
  for (int e = 0; e < 16; ++e) {  // rolled: the path of a mismatch costs the healthy one no register
    const Bits g = mfma_wide_pick<T>(got, e), w = want(e);
    if (g != w) {
      ++bad;
      if (*mine < MFMA_CHECK_RECORDS) {  // a lane asks for at most 16 slots however long it runs
        ++*mine;
        const unsigned slot = atomicAdd(nrec, 1u);
        if (slot < MFMA_CHECK_RECORDS) {
          uint32_t g32, w32;
          T::record_words(g, w, &g32, &w32);
          recs[slot] = MfmaCheckRecord{blockIdx.x, static_cast<uint32_t>(T::row(e)), static_cast<uint32_t>(T::col(e)),
                                       static_cast<uint32_t>(round), g32, w32};
        }
      }
    }
  }
  return bad;
}

// The check of mfma_check_kernel on format T at K = T::CHECK_K. rounds >= 1; flip_pos holds
// MFMA_CHECK_MAX_FLIPS entries. Round 0 is compared one output at a time with the integer reference
// (no second vector of 16 values: the fp64 accumulators and the kept anchor already take 64 registers),
// later rounds bitwise with the kept round-0 accumulators.
// dbg_block >= 0: that workgroup also stores its A[64 x k], B[k x 64] and round-0 C[64 x 64] as
// doubles, which hold every value of either format exactly (tests only).
template <class T>
__global__ __launch_bounds__(256, T::CHECK_WG_PER_CU) void mfma_check_wide_kernel(
    uint32_t seed, int rounds, int flips, const uint32_t* __restrict__ flip_pos, unsigned long long* __restrict__ errors,
    unsigned* __restrict__ nrec, MfmaCheckRecord* __restrict__ recs, int dbg_block, double* __restrict__ dbg_a,
    double* __restrict__ dbg_b, double* __restrict__ dbg_c) {
  typedef typename T::Elem Elem;
  typedef typename T::Acc Acc;
  constexpr int K = T::CHECK_K, LD = K + T::PAD, STEPS = K / T::KSTEP;
  __shared__ __attribute__((aligned(16))) Elem As[MFMA_TILE * LD];  // 2 x 17 KiB for either format
  __shared__ __attribute__((aligned(16))) Elem Bt[MFMA_TILE * LD];
  // uniform: never index past the flip table, never loop on a non-positive stride
  if (rounds < 1 || flips < 0 || flips > MFMA_CHECK_MAX_FLIPS) return;
  const int t = threadIdx.x;
  constexpr uint32_t nb = MFMA_TILE * K;
  for (uint32_t idx = t; idx < nb; idx += 256) {
    const uint32_t i = idx / K, k = idx - i * K;
    As[i * LD + k] = T::check_value(seed, blockIdx.x, idx);                       // A[i][k]
    Bt[i * LD + k] = T::check_value(seed, blockIdx.x, nb + k * MFMA_TILE + i);   // B[k][i]
  }
  __syncthreads();
  const bool dbg = static_cast<int>(blockIdx.x) == dbg_block;
  if (dbg)
    for (uint32_t idx = t; idx < nb; idx += 256) {
      const uint32_t i = idx / K, k = idx - i * K;
      dbg_a[i * K + k] = static_cast<double>(As[i * LD + k]);
      dbg_b[k * MFMA_TILE + i] = static_cast<double>(Bt[i * LD + k]);
    }

  // round 0: the MFMA product against integer VALU arithmetic on the same LDS operands
  const Acc anchor = T::slice(As, Bt, LD, STEPS, mfma_wide_zero<T>());
  if (dbg) {
#pragma unroll
    for (int e = 0; e < 16; ++e) dbg_c[T::row(e) * MFMA_TILE + T::col(e)] = static_cast<double>(T::value(anchor, e));
  }
  unsigned mine = 0;
  unsigned long long bad = mfma_wide_compare<T, 1>(
      anchor, [&](int e) { return T::reference(As + T::row(e) * LD, Bt + T::col(e) * LD); },
      mfma_wide_flip_mask<T>(0, rounds, flips, flip_pos), 0, nrec, recs, &mine);

  // rounds 1..: re-read the operands, recompute, compare bitwise with the kept round-0 accumulators
  for (int round = 1; round < rounds; ++round) {
    asm volatile("" ::: "memory");  // the operands are read from LDS again, the product is not reused
    const Acc c = T::slice(As, Bt, LD, STEPS, mfma_wide_zero<T>());
    bad += mfma_wide_compare<T, 16>(c, [&](int e) { return mfma_wide_pick<T>(anchor, e); },
                                    mfma_wide_flip_mask<T>(round, rounds, flips, flip_pos), round, nrec, recs, &mine);
  }
  if (bad) atomicAdd(errors, bad);  // one per lane that saw a mismatch: none on a healthy part
}

// ---------------------------------------------------------------------------- runners
template <class T>
inline void mfma_check_wide_launch(const MfmaCheckRun& run, int rounds, int flips, int dbg_block, void* dbg_a, void* dbg_b,
                                   void* dbg_c) {
  hipLaunchKernelGGL(mfma_check_wide_kernel<T>, dim3(run.blocks), dim3(256), 0, 0, run.seed, rounds, flips,
                     run.flip_pos.as<const uint32_t>(), run.errors.as<unsigned long long>(), run.nrec.as<unsigned>(),
                     run.recs.as<MfmaCheckRecord>(), dbg_block, static_cast<double*>(dbg_a), static_cast<double*>(dbg_b),
                     static_cast<double*>(dbg_c));
}

inline bool mfma_fmt_is_wide(int fmt) { return fmt == MFMA_WIDE_FP64 || fmt == MFMA_WIDE_INT8; }

// (the table over every format of the check, mfma_check_fmt_ops, and what runs on it: mfma_check_sparse.h)

inline size_t mfma_wide_tiles(int m, int n, int k, int kstep) {
  if (m <= 0 || n <= 0 || m % MFMA_TILE || n % MFMA_TILE)
    throw std::invalid_argument("M and N must be positive multiples of 64");
  if (k <= 0 || k % kstep) throw std::invalid_argument("K must be a positive multiple of " + std::to_string(kstep));
  const size_t tiles = static_cast<size_t>(m / MFMA_TILE) * (n / MFMA_TILE);
  if (tiles > 0x7fffffffu) throw std::invalid_argument("too many tiles for one launch");
  return tiles;
}

// C[m x n] = A[m x k] * B[k x n], row-major fp64
inline std::vector<double> mfma_gemm_fp64_host(const std::vector<double>& a, const std::vector<double>& b, int m, int n, int k,
                                               int dev) {
  const size_t tiles = mfma_wide_tiles(m, n, k, MfmaWideFp64::KSTEP);
  if (a.size() != static_cast<size_t>(m) * k || b.size() != static_cast<size_t>(k) * n)
    throw std::invalid_argument("A must be MxK and B KxN fp64");
  AK_HIP(hipSetDevice(dev));
  DevBuf da(a), db(b), dc(static_cast<size_t>(m) * n * sizeof(double));
  dc.fill(0xff);  // NaN: a value the kernel never wrote cannot pass
  hipLaunchKernelGGL(mfma_gemm_fp64_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, da.as<const double>(),
                     db.as<const double>(), dc.as<double>(), m, n, k);
  AK_HIP(hipGetLastError());
  return dc.download<double>();
}

// C[m x n] int32 = A[m x k] * B[k x n], row-major int8; transposes B for the kernel
inline std::vector<int> mfma_gemm_int8_host(const std::vector<int8_t>& a, const std::vector<int8_t>& b, int m, int n, int k,
                                            int dev) {
  const size_t tiles = mfma_wide_tiles(m, n, k, MfmaWideInt8::KSTEP);
  if (a.size() != static_cast<size_t>(m) * k || b.size() != static_cast<size_t>(k) * n)
    throw std::invalid_argument("A must be MxK and B KxN int8");
  std::vector<int8_t> bt(b.size());
  for (size_t j = 0; j < static_cast<size_t>(n); ++j)
    for (size_t kk = 0; kk < static_cast<size_t>(k); ++kk) bt[j * k + kk] = b[kk * n + j];
  AK_HIP(hipSetDevice(dev));
  DevBuf da(a), db(bt), dc(static_cast<size_t>(m) * n * sizeof(int));
  dc.fill(0xff);
  hipLaunchKernelGGL(mfma_gemm_int8_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, 0, da.as<const int8_t>(),
                     db.as<const int8_t>(), dc.as<int>(), m, n, k);
  AK_HIP(hipGetLastError());
  return dc.download<int>();
}

}  // namespace amdkube
