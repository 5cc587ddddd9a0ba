// Per-CU integrity check: an LDS march over the whole 160 KiB, a cross-check of the vector ALU
// pipes, an agreement check of the transcendental unit, and the physical place of every workgroup.
// Behind cu-check, the device plugin's cu health probe and hip.cu_check. gpu_common.h provides
// mix32 (one- and three-argument), v4u and the host plumbing.
//
// A workgroup of cu_check_kernel declares all 163,840 B of LDS, so it has its CU to itself: one
// workgroup is one CU for its lifetime, and the location wave 0 reads at entry is the location of
// everything the workgroup computes. The disciplines of mfma_check.h hold: every loop is bounded,
// arguments are validated at entry with a uniform return, there is no inter-workgroup
// synchronisation, the units mask is uniform so every __syncthreads sits in uniform control flow,
// errors are one atomicAdd per lane that saw a mismatch and at most 16 records are kept.
//
// Formulas (amdkube/ops/cucheck.py is written from these, not from the device):
//   key(tag)     = mix32(seed, block, tag), the three-argument mix32 of gpu_common.h
//   lds          word address wa in [0, 40960) (byte address 4 wa), round r:
//                k = key(0x4c000000 + r), mul = k | 1, add = mix32(k ^ 0x85ebca6b),
//                P(wa) = wa * mul + add (mod 2^32; mul is odd, so P is a bijection of wa).
//                Pass 1 writes P ascending, pass 2 verifies P and writes ~P ascending, pass 3
//                verifies ~P and writes P descending, pass 4 verifies P. The 160 KiB are 10,240
//                16-byte slots; in pass p lane t of the workgroup owns slots 1024 j + ((t + 64 (p-1)) & 1023),
//                j = 0..9, so wave w verifies what wave w+1 wrote.
//   valu         lane t, h_n = key(0x56000000 + 8 t + n):
//                a0 = h0 & 0xfff, b0 = (h0 >> 12) & 0x7ff, c0 = h1 & 0x7fffff, (a1, b1, c1) from h2, h3
//                alike: a < 2^12, b < 2^11, c < 2^23, so a b + c < 2^24 is exact in fp32 (with b up
//                to 2^12 the sum reaches 2^24 + 2^23 and odd values there are not fp32 numbers).
//                Computed as v_fma_f32, v_pk_fma_f32, v_fma_f64 (the compiler picks its two-operand
//                encoding, v_fmac_f64) and integer multiply-add (v_mad_u32_u24).
//                wide: (h4, h5, h6) & 0x3ffffff, wa wb + wc < 2^53 in v_fma_f64 against 64-bit integers.
//                chain: x = h7, 16 times x = x * (h4 | 1) + h5 (mod 2^32).
//   trans        lane l of wave w, g = 64 (w >> 1) + l, h = key(0x54000000 + 32 g + 4 f + s), s = 0..3:
//                f = 0 exp2: x = (int((h * 10485760) >> 32) - 5242880) * 2^-18, in [-20, 20)
//                f = 1 log2: i = ((h >> 23) * 38) >> 9, exponent i - 20 (i < 19) or i - 18, mantissa
//                            h & 0x7fffff: [2^-20, 2^-1) and [2, 2^20). The binades next to 1 are left
//                            out: there the result is near 0 and the unit's error is a large count of
//                            ulps of it, which a bound in ulps cannot express.
//                f = 2, 3, 4 rcp, rsq, sqrt: exponent (((h >> 23) * 40) >> 9) - 20, mantissa h & 0x7fffff.
//   digest       d = 0x811c9dc5, then d = (d ^ x) * 0x01000193 for every result word x in order.
//
// Location. HW_REG_HW_ID: WAVE_ID [3:0], SIMD_ID [5:4], PIPE_ID [7:6], CU_ID [11:8], SH_ID [12],
// SE_ID [15:13], TG_ID [19:16], VM_ID [23:20], QUEUE_ID [26:24], STATE_ID [29:27], ME_ID [31:30];
// HW_REG_XCC_ID: XCC_ID [3:0]. A location is (xcc, se, sh, cu).
// Observed on an MI355X (256 CUs), 1024 workgroups of one launch: these masks give exactly 256 distinct
// locations, 32 on each of the XCDs 0..7 and four workgroups on every one of them; SE_ID takes 0..3,
// SH_ID only 0, and CU_ID nine values, 0..8 (a shader engine has more CU slots than active CUs, so the
// ids are not dense). Of the other HW_ID fields only SIMD_ID varied (wave 0 of a workgroup starts on
// any SIMD: with it the words give 1015 distinct values, so a mask that took it in would overcount);
// WAVE_ID, PIPE_ID, TG_ID and STATE_ID read 0, VM_ID, QUEUE_ID and ME_ID one constant each. XCC_ID
// bits [31:4] read 0. One launch of 4 workgroups per CU covered every CU in the runs measured.
#pragma once

#include <map>
#include <set>

#include "gpu_common.h"

namespace amdkube {

constexpr int CU_CHECK_LDS_BYTES = 163840;
constexpr int CU_CHECK_SLOTS = CU_CHECK_LDS_BYTES / 16;  // 10,240 16-byte slots
constexpr int CU_CHECK_WORDS = CU_CHECK_LDS_BYTES / 4;   // 40,960 words
constexpr int CU_CHECK_THREADS = 1024;
constexpr int CU_CHECK_SLOTS_PER_LANE = CU_CHECK_SLOTS / CU_CHECK_THREADS;  // 10
constexpr int CU_CHECK_BLOCKS_PER_CU = 4;
constexpr int CU_CHECK_RECORDS = 16;
constexpr int CU_CHECK_MAX_FLIPS = 4096;
constexpr int CU_CHECK_EXTRA_LAUNCHES = 3;  // added one by one while a run has not seen every CU
constexpr int CU_CHECK_CHAIN = 16;
constexpr int CU_CHECK_TRANS_FUNCS = 5, CU_CHECK_TRANS_SETS = 4;
constexpr int CU_CHECK_TRANS_N = CU_CHECK_TRANS_FUNCS * CU_CHECK_TRANS_SETS;  // 20 values per lane
constexpr int CU_CHECK_VALU_OPS = 12;   // dumped operand words per lane: a0 b0 c0 a1 b1 c1 wa wb wc x m k
constexpr int CU_CHECK_VALU_MADS = 2 + 2 + 2 + 2 + 2 + CU_CHECK_CHAIN;  // multiply-adds per lane and round
enum : int { CU_UNIT_LDS = 1, CU_UNIT_VALU = 2, CU_UNIT_TRANS = 4, CU_UNIT_ALL = 7 };
// (CU_HWREG_HW_ID, CU_HWREG_XCC_ID, CuLocation and cu_decode_location: gpu_common.h, shared with hbm_check.h)

// unit: 0 lds, 1 valu, 2 trans; hw_id and xcc_id are the raw words of the wave that saw the mismatch.
// lds: index is the LDS byte address and pass the march pass (2, 3 or 4). valu: index is
// 8 * lane + the compared value (0, 1 fp32; 2, 3 packed fp32; 4, 5 fp64; 6 wide fp64; 7 the digest
// of a later round), a 64-bit value shows the differing half. trans: index is the lane, got and want
// the digests (round 0: of the partner wave, later: of round 0).
struct CuCheckRecord {
  uint32_t unit, block, round, index, pass, got, want, hw_id, xcc_id;
};

struct CuCheckArgs {
  uint32_t seed;
  int rounds, flips, units, dbg_block;
  const uint32_t* flip_pos;            // CU_CHECK_MAX_FLIPS positions, see CuCheckRun
  unsigned long long* errors;          // [3]: lds, valu, trans
  unsigned* block_errors;              // [blocks]
  unsigned* nrec;
  CuCheckRecord* recs;                 // [CU_CHECK_RECORDS]
  uint32_t* loc;                       // [blocks][2]: raw HW_ID, XCC_ID
  // dbg_block >= 0: that workgroup also stores (tests only)
  v4u* dbg_lds;                        // [10240] the image read back after pass 1 of round 0
  uint32_t* dbg_valu_ops;              // [1024][12]
  float* dbg_valu_f32;                 // [1024][4]: fp32 0, 1, packed 0, 1
  double* dbg_valu_f64;                // [1024][3]: fp64 0, 1, wide
  unsigned long long* dbg_valu_int;    // [1024][4]: integer 0, 1, wide, chain
  float* dbg_trans_in;                 // [1024][20]
  float* dbg_trans_out;                // [1024][20]
};

struct CuCheckCtx {
  const CuCheckArgs* a;
  int round;
  unsigned mine;  // record slots this lane has asked for
};

// out of line: the mismatch path is never taken on a healthy part and must not cost the march registers
// (everything by value, so nothing of the kernel has to live in memory for it)
__device__ __noinline__ void cu_check_store_record(unsigned* nrec, CuCheckRecord* recs, uint32_t unit_pass, uint32_t round,
                                                   uint32_t index, uint32_t got, uint32_t want) {
  const unsigned slot = atomicAdd(nrec, 1u);
  if (slot < CU_CHECK_RECORDS)
    recs[slot] = CuCheckRecord{unit_pass >> 8, blockIdx.x, round, index, unit_pass & 255u, got, want,
                               __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID), __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID)};
}

__device__ __forceinline__ void cu_check_record(CuCheckCtx& cx, uint32_t unit, uint32_t index, uint32_t pass, uint32_t got,
                                                uint32_t want) {
  if (cx.mine >= CU_CHECK_RECORDS) return;  // a lane asks for at most 16 slots however long it runs
  ++cx.mine;
  cu_check_store_record(cx.a->nrec, cx.a->recs, unit << 8 | pass, static_cast<uint32_t>(cx.round), index, got, want);
}

// the value is what it was, but the compiler no longer knows it: every round recomputes
__device__ __forceinline__ uint32_t cu_launder(uint32_t x) {
  asm volatile("" : "+v"(x));
  return x;
}

__device__ __forceinline__ float cu_launder(float x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ double cu_launder(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

__device__ __forceinline__ uint32_t cu_digest(uint32_t d, uint32_t x) { return (d ^ x) * 0x01000193u; }

// Self-test flips of `round` that belong to the unit in slot `us` of the `n_en` enabled units: flip i
// goes to unit slot i mod n_en and round (i / n_en) mod rounds, at position flip_pos[i] = block * elems +
// element (distinct positions, chosen by the host). The lds flips are spread over the verify passes
// 2 + (i / n_en / rounds) mod 3. At most CU_CHECK_MAX_FLIPS iterations.
template <class F>
__device__ __forceinline__ void cu_check_flips(const CuCheckArgs& a, int round, int us, int n_en, uint32_t elems, F&& hit) {
  for (int q = round; q * n_en + us < a.flips; q += a.rounds) {
    const uint32_t p = a.flip_pos[q * n_en + us], b = p / elems;
    if (b == blockIdx.x) hit(p - b * elems, static_cast<uint32_t>(q / a.rounds));
  }
}

// ---------------------------------------------------------------------------- lds
// One pass of the march over this lane's 10 slots. kVerify: compare with P ^ inv first; kWrite: store
// (kVerify ? ~(P ^ inv) : P). fm: self-test mask over the lane's 40 compared words (bit 4 j + c),
// XORed into the compared copy only. Returns the mismatching words.
template <bool kVerify, bool kWrite, bool kFlip>
__device__ __forceinline__ unsigned cu_lds_pass(v4u* img, int pass, bool descending, uint32_t inv, uint32_t mul, uint32_t add,
                                                unsigned long long fm, CuCheckCtx& cx) {
  // laundered, so the slot addresses and pattern bases of all four passes are worked out here, one
  // multiply per pass, and not kept in registers across the rounds
  const uint32_t tp = cu_launder((threadIdx.x + 64u * (pass - 1)) & (CU_CHECK_THREADS - 1));
  const uint32_t base = (tp * 4u) * mul + add, step = (4u * CU_CHECK_THREADS) * mul;
  unsigned bad = 0;
#pragma unroll 5
  for (int jj = 0; jj < CU_CHECK_SLOTS_PER_LANE; ++jj) {
    const int j = descending ? CU_CHECK_SLOTS_PER_LANE - 1 - jj : jj;
    const uint32_t slot = j * CU_CHECK_THREADS + tp;
    const uint32_t p0 = base + j * step;
    const v4u want = v4u{p0, p0 + mul, p0 + 2u * mul, p0 + 3u * mul} ^ inv;
    if (kVerify) {
      v4u got = img[slot];
      if (kFlip) {
        const uint32_t f = static_cast<uint32_t>(fm >> (4 * j)) & 15u;
        got ^= v4u{f & 1u, (f >> 1) & 1u, (f >> 2) & 1u, (f >> 3) & 1u};
      }
      const v4u d = got ^ want;
      if ((d.x | d.y | d.z | d.w) != 0) {  // the healthy path: one branch per slot
#pragma unroll 1
        for (uint32_t c = 0; c < 4; ++c) {  // rolled up, with selects: small code on a path that is never taken
          const uint32_t g = c == 0 ? got.x : c == 1 ? got.y : c == 2 ? got.z : got.w;
          const uint32_t e = c == 0 ? want.x : c == 1 ? want.y : c == 2 ? want.z : want.w;
          if (g != e) {
            ++bad;
            cu_check_record(cx, 0, slot * 16u + 4u * c, pass, g, e);
          }
        }
      }
    }
    if (kWrite) img[slot] = kVerify ? ~want : want;
  }
  return bad;
}

template <bool kFlip>
__device__ __forceinline__ unsigned long long cu_lds_flip_mask(const CuCheckArgs& a, int round, int us, int n_en, int pass) {
  unsigned long long m = 0;
  if (kFlip) {
    const uint32_t tp = (threadIdx.x + 64u * (pass - 1)) & (CU_CHECK_THREADS - 1);
    cu_check_flips(a, round, us, n_en, CU_CHECK_WORDS, [&](uint32_t word, uint32_t q) {
      const uint32_t slot = word >> 2;
      if (2 + static_cast<int>(q % 3u) == pass && (slot & (CU_CHECK_THREADS - 1)) == tp)
        m |= 1ull << (4 * (slot / CU_CHECK_THREADS) + (word & 3u));
    });
  }
  return m;
}

template <bool kFlip>
__device__ __forceinline__ unsigned cu_lds_round(v4u* img, const CuCheckArgs& a, int us, int n_en, CuCheckCtx& cx, bool dbg) {
  const uint32_t k = mix32(a.seed, blockIdx.x, 0x4c000000u + static_cast<uint32_t>(cx.round));
  const uint32_t mul = k | 1u, add = mix32(k ^ 0x85ebca6bu);
  unsigned bad = 0;
  cu_lds_pass<false, true, false>(img, 1, false, 0u, mul, add, 0, cx);
  __syncthreads();
  if (dbg && cx.round == 0) {  // read back by the lanes that verify it in pass 2
    const uint32_t tp = (threadIdx.x + 64u) & (CU_CHECK_THREADS - 1);
    for (int j = 0; j < CU_CHECK_SLOTS_PER_LANE; ++j) a.dbg_lds[j * CU_CHECK_THREADS + tp] = img[j * CU_CHECK_THREADS + tp];
  }
  bad += cu_lds_pass<true, true, kFlip>(img, 2, false, 0u, mul, add, cu_lds_flip_mask<kFlip>(a, cx.round, us, n_en, 2), cx);
  __syncthreads();
  bad += cu_lds_pass<true, true, kFlip>(img, 3, true, ~0u, mul, add, cu_lds_flip_mask<kFlip>(a, cx.round, us, n_en, 3), cx);
  __syncthreads();
  bad += cu_lds_pass<true, false, kFlip>(img, 4, false, 0u, mul, add, cu_lds_flip_mask<kFlip>(a, cx.round, us, n_en, 4), cx);
  __syncthreads();  // the image is free for the next unit
  return bad;
}

// ---------------------------------------------------------------------------- valu
typedef float v2f __attribute__((ext_vector_type(2)));

struct CuValuOps {
  uint32_t a0, b0, c0, a1, b1, c1, wa, wb, wc, x, m, k;
};

__device__ __forceinline__ CuValuOps cu_valu_operands(uint32_t seed) {
  uint32_t h[8];
#pragma unroll
  for (int n = 0; n < 8; ++n) h[n] = mix32(seed, blockIdx.x, 0x56000000u + 8u * threadIdx.x + n);
  return CuValuOps{h[0] & 0xfffu, (h[0] >> 12) & 0x7ffu, h[1] & 0x7fffffu, h[2] & 0xfffu, (h[2] >> 12) & 0x7ffu,
                   h[3] & 0x7fffffu, h[4] & 0x3ffffffu, h[5] & 0x3ffffffu, h[6] & 0x3ffffffu, h[7], h[4] | 1u, h[5]};
}

__device__ __forceinline__ uint32_t cu_hi(double x) { return static_cast<uint32_t>(__double_as_longlong(x) >> 32); }
__device__ __forceinline__ uint32_t cu_lo(double x) { return static_cast<uint32_t>(__double_as_longlong(x)); }

// One round of the valu unit. Round 0 compares the pipes with each other (all against the integer
// result) and keeps the digest in *digest0; later rounds compare their digest with it. flip XORs the low
// bit of the compared copy of the first fp32 result (round 0) or of the digest (later rounds).
__device__ __forceinline__ unsigned cu_valu_round(const CuCheckArgs& a, bool flip, uint32_t* digest0, CuCheckCtx& cx,
                                                  bool dbg) {
  const CuValuOps o = cu_valu_operands(cu_launder(a.seed));  // hashed again every round: nothing is carried over
  const uint32_t a0 = o.a0, b0 = o.b0, c0 = o.c0, a1 = o.a1, b1 = o.b1, c1 = o.c1, wa = o.wa, wb = o.wb, wc = o.wc;
  // The converted operands are laundered: knowing that they are small integers, the compiler otherwise
  // replaces every floating-point form by the integer multiply-add and a conversion.
  const float fa0 = cu_launder(static_cast<float>(a0)), fb0 = cu_launder(static_cast<float>(b0));
  const float fa1 = cu_launder(static_cast<float>(a1)), fb1 = cu_launder(static_cast<float>(b1));
  const float fc0 = cu_launder(static_cast<float>(c0)), fc1 = cu_launder(static_cast<float>(c1));
  float f0, f1;  // written out: left to itself the compiler packs the two into one v_pk_fma_f32
  asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(f0) : "v"(fa0), "v"(fb0), "v"(fc0));
  asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(f1) : "v"(fa1), "v"(fb1), "v"(fc1));
  v2f pk;
  {  // the same operands in fresh registers, so the packed form is not merged with the scalar one
    v2f pa = {fa0, fa1}, pb = {fb0, fb1}, pc = {fc0, fc1};
    asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(pk) : "v"(pa), "v"(pb), "v"(pc));
  }
  const double d0 = __builtin_fma(cu_launder(static_cast<double>(a0)), cu_launder(static_cast<double>(b0)),
                                  cu_launder(static_cast<double>(c0)));
  const double d1 = __builtin_fma(cu_launder(static_cast<double>(a1)), cu_launder(static_cast<double>(b1)),
                                  cu_launder(static_cast<double>(c1)));
  const uint32_t i0 = a0 * b0 + c0, i1 = a1 * b1 + c1;
  const double dw = __builtin_fma(cu_launder(static_cast<double>(wa)), cu_launder(static_cast<double>(wb)),
                                  cu_launder(static_cast<double>(wc)));
  const unsigned long long iw = static_cast<unsigned long long>(wa) * wb + wc;
  uint32_t x = o.x;
  const uint32_t m = o.m, k = o.k;
#pragma unroll
  for (int s = 0; s < CU_CHECK_CHAIN; ++s) x = x * m + k;

  uint32_t d = 0x811c9dc5u;
  d = cu_digest(d, __float_as_uint(f0));
  d = cu_digest(d, __float_as_uint(f1));
  d = cu_digest(d, __float_as_uint(pk.x));
  d = cu_digest(d, __float_as_uint(pk.y));
  d = cu_digest(cu_digest(d, cu_lo(d0)), cu_hi(d0));
  d = cu_digest(cu_digest(d, cu_lo(d1)), cu_hi(d1));
  d = cu_digest(d, i0);
  d = cu_digest(d, i1);
  d = cu_digest(cu_digest(d, cu_lo(dw)), cu_hi(dw));
  d = cu_digest(cu_digest(d, static_cast<uint32_t>(iw)), static_cast<uint32_t>(iw >> 32));
  d = cu_digest(d, x);

  const uint32_t t = threadIdx.x;
  unsigned bad = 0;
  if (cx.round == 0) {
    *digest0 = d;
    if (dbg) {
      const uint32_t ops[CU_CHECK_VALU_OPS] = {a0, b0, c0, a1, b1, c1, wa, wb, wc, o.x, m, k};
#pragma unroll
      for (int n = 0; n < CU_CHECK_VALU_OPS; ++n) a.dbg_valu_ops[t * CU_CHECK_VALU_OPS + n] = ops[n];
      a.dbg_valu_f32[t * 4 + 0] = f0;
      a.dbg_valu_f32[t * 4 + 1] = f1;
      a.dbg_valu_f32[t * 4 + 2] = pk.x;
      a.dbg_valu_f32[t * 4 + 3] = pk.y;
      a.dbg_valu_f64[t * 3 + 0] = d0;
      a.dbg_valu_f64[t * 3 + 1] = d1;
      a.dbg_valu_f64[t * 3 + 2] = dw;
      a.dbg_valu_int[t * 4 + 0] = i0;
      a.dbg_valu_int[t * 4 + 1] = i1;
      a.dbg_valu_int[t * 4 + 2] = iw;
      a.dbg_valu_int[t * 4 + 3] = x;
    }
    const uint32_t w0 = __float_as_uint(static_cast<float>(i0)), w1 = __float_as_uint(static_cast<float>(i1));
    const uint32_t g[4] = {__float_as_uint(f0) ^ (flip ? 1u : 0u), __float_as_uint(f1), __float_as_uint(pk.x),
                           __float_as_uint(pk.y)};
    const uint32_t e[4] = {w0, w1, w0, w1};
    const double dg[3] = {d0, d1, dw};
    const double de[3] = {static_cast<double>(i0), static_cast<double>(i1), static_cast<double>(iw)};
    uint32_t diff = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) diff |= g[n] ^ e[n];
#pragma unroll
    for (int n = 0; n < 3; ++n) diff |= (cu_lo(dg[n]) ^ cu_lo(de[n])) | (cu_hi(dg[n]) ^ cu_hi(de[n]));
    if (diff) {  // the healthy path: one branch per round
#pragma unroll
      for (int n = 0; n < 4; ++n)
        if (g[n] != e[n]) {
          ++bad;
          cu_check_record(cx, 1, 8u * t + n, 0, g[n], e[n]);
        }
#pragma unroll
      for (int n = 0; n < 3; ++n)
        if (__double_as_longlong(dg[n]) != __double_as_longlong(de[n])) {
          ++bad;
          const bool low = cu_lo(dg[n]) != cu_lo(de[n]);
          cu_check_record(cx, 1, 8u * t + 4 + n, 0, low ? cu_lo(dg[n]) : cu_hi(dg[n]), low ? cu_lo(de[n]) : cu_hi(de[n]));
        }
    }
  } else {
    const uint32_t g = d ^ (flip ? 1u : 0u);
    if (g != *digest0) {
      ++bad;
      cu_check_record(cx, 1, 8u * t + 7, 0, g, *digest0);
    }
  }
  return bad;
}

// ---------------------------------------------------------------------------- trans
__device__ __forceinline__ float cu_trans_input(uint32_t seed, uint32_t g, int f, int s) {
  const uint32_t h = mix32(seed, blockIdx.x, 0x54000000u + 32u * g + 4u * f + s);
  if (f == 0) {
    const int v = static_cast<int>((static_cast<unsigned long long>(h) * 10485760ull) >> 32) - 5242880;
    return static_cast<float>(v) * 0x1p-18f;  // |v| < 2^23: exact
  }
  uint32_t e;
  if (f == 1) {
    const uint32_t i = ((h >> 23) * 38u) >> 9;
    e = i < 19u ? 107u + i : 109u + i;
  } else {
    e = 107u + (((h >> 23) * 40u) >> 9);
  }
  return __uint_as_float((e << 23) | (h & 0x7fffffu));
}

__device__ __forceinline__ float cu_trans_apply(int f, float x) {
  switch (f) {
    case 0: return __builtin_amdgcn_exp2f(x);
    case 1: return __builtin_amdgcn_logf(x);
    case 2: return __builtin_amdgcn_rcpf(x);
    case 3: return __builtin_amdgcn_rsqf(x);
    default: return __builtin_amdgcn_sqrtf(x);
  }
}

// One round of the trans unit. Waves w and w^1 compute the same 20 values; in round 0 they exchange
// digests through LDS word `lane of the workgroup` and must agree, later rounds must match round 0.
// flip XORs the low bit of this lane's compared copy of its own digest.
__device__ __forceinline__ unsigned cu_trans_round(uint32_t* lds_words, const CuCheckArgs& a, bool flip, uint32_t* digest0,
                                                   CuCheckCtx& cx, bool dbg) {
  const uint32_t t = threadIdx.x, g = 64u * (t >> 7) + (t & 63u);
  const uint32_t seed = cu_launder(a.seed);  // hashed again every round: nothing is carried over
  uint32_t d = 0x811c9dc5u;
#pragma unroll
  for (int f = 0; f < CU_CHECK_TRANS_FUNCS; ++f)
#pragma unroll
    for (int s = 0; s < CU_CHECK_TRANS_SETS; ++s) {
      const float x = cu_trans_input(seed, g, f, s);
      const float y = cu_trans_apply(f, x);
      d = cu_digest(d, __float_as_uint(y));
      if (dbg && cx.round == 0) {
        a.dbg_trans_in[t * CU_CHECK_TRANS_N + f * CU_CHECK_TRANS_SETS + s] = x;
        a.dbg_trans_out[t * CU_CHECK_TRANS_N + f * CU_CHECK_TRANS_SETS + s] = y;
      }
    }
  const uint32_t mine = d ^ (flip ? 1u : 0u);
  uint32_t want;
  if (cx.round == 0) {  // uniform
    *digest0 = d;
    lds_words[t] = d;
    __syncthreads();
    want = lds_words[t ^ 64u];
    __syncthreads();
  } else {
    want = *digest0;
  }
  if (mine == want) return 0;
  cu_check_record(cx, 2, t, 0, mine, want);
  return 1;
}

// ---------------------------------------------------------------------------- the kernel
// kFlip: the self-test is on; kDbg: some workgroup dumps (never both: the dump launch has no flips)
template <bool kFlip, bool kDbg>
__device__ __forceinline__ void cu_check_body(v4u* img, const CuCheckArgs& a) {
  const bool dbg = kDbg && static_cast<int>(blockIdx.x) == a.dbg_block;
  const int n_en = __builtin_popcount(static_cast<unsigned>(a.units));
  const int us_lds = 0, us_valu = a.units & CU_UNIT_LDS ? 1 : 0, us_trans = n_en - 1;
  CuCheckCtx cx{&a, 0, 0};
  uint32_t valu0 = 0, trans0 = 0;
  unsigned bad[3] = {0, 0, 0};
  for (int round = 0; round < a.rounds; ++round) {
    cx.round = round;
    if (a.units & CU_UNIT_LDS) bad[0] += cu_lds_round<kFlip>(img, a, us_lds, n_en, cx, dbg);
    if (a.units & CU_UNIT_VALU) {
      bool flip = false;
      if (kFlip)
        cu_check_flips(a, round, us_valu, n_en, CU_CHECK_THREADS, [&](uint32_t lane, uint32_t) { flip |= lane == threadIdx.x; });
      bad[1] += cu_valu_round(a, flip, &valu0, cx, dbg);
    }
    if (a.units & CU_UNIT_TRANS) {
      bool flip = false;
      if (kFlip)
        cu_check_flips(a, round, us_trans, n_en, CU_CHECK_THREADS, [&](uint32_t lane, uint32_t) { flip |= lane == threadIdx.x; });
      bad[2] += cu_trans_round(reinterpret_cast<uint32_t*>(img), a, flip, &trans0, cx, dbg);
    }
  }
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (bad[u]) {  // one per lane that saw a mismatch: none on a healthy part
      atomicAdd(a.errors + u, static_cast<unsigned long long>(bad[u]));
      atomicAdd(a.block_errors + blockIdx.x, bad[u]);
    }
}

__global__ __launch_bounds__(CU_CHECK_THREADS) void cu_check_kernel(CuCheckArgs a) {
  __shared__ __attribute__((aligned(16))) v4u img[CU_CHECK_SLOTS];
  // uniform: never index past the flip table, never loop on a non-positive stride
  if (a.rounds < 1 || a.flips < 0 || a.flips > CU_CHECK_MAX_FLIPS || a.units < 1 || a.units > CU_UNIT_ALL) return;
  if (threadIdx.x == 0) {  // wave 0 reads the place once, lane 0 stores it
    a.loc[2 * blockIdx.x] = __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID);
    a.loc[2 * blockIdx.x + 1] = __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID);
  }
  if (a.flips > 0)
    cu_check_body<true, false>(img, a);
  else if (a.dbg_block >= 0)
    cu_check_body<false, true>(img, a);
  else
    cu_check_body<false, false>(img, a);
}

// ---------------------------------------------------------------------------- runners
inline int cu_check_blocks(int cu_count) { return (cu_count > 0 ? cu_count : 256) * CU_CHECK_BLOCKS_PER_CU; }

// unit u has the mask bit 1 << u and the number u in a record
constexpr const char* CU_UNIT_NAMES[3] = {"lds", "valu", "trans"};

// "lds,valu,trans" -> mask; throws std::invalid_argument on an unknown or empty name
inline int cu_check_units(const std::string& list) {
  int mask = 0;
  for (const std::string& name : split_list(list)) {
    int u = 0;
    while (u < 3 && name != CU_UNIT_NAMES[u]) ++u;
    if (u == 3) throw std::invalid_argument("unknown unit '" + name + "': expected a comma list over lds, valu, trans");
    mask |= 1 << u;
  }
  return mask;
}

struct CuCheckBadCu {
  CuLocation where;
  unsigned long long errors = 0;
};

struct CuCheckResult {
  double ms = 0, lds_gbps = 0, valu_gops = 0;
  long long rounds = 0;
  int blocks = 0, units = 0, launches = 0;
  int cus = 0, cus_covered = 0, xccs = 0;
  unsigned long long errors = 0, errors_by_unit[3] = {0, 0, 0};
  std::vector<CuLocation> locations;      // the distinct places seen over all launches, sorted
  std::vector<uint32_t> block_loc;        // [blocks][2] raw HW_ID, XCC_ID of the timed launch
  std::vector<CuCheckBadCu> bad_cus;      // at most 16
  std::vector<CuCheckRecord> first_errors;
};

// Device buffers and the launch of one check; errors and records accumulate over launches, the
// places and per-workgroup error counts are collected after each launch.
struct CuCheckRun {
  int cus, blocks, units;
  uint32_t seed;
  DevBuf errors, block_errors, nrec, recs, flip_pos, loc;
  std::set<uint32_t> seen;
  std::map<uint32_t, unsigned long long> bad;
  std::vector<uint32_t> block_loc;
  int launches = 0;
  CuCheckRun(int dev, uint32_t seed_, int units_)
      : cus(dev_info(dev).cu_count), blocks(cu_check_blocks(cus)), units(checked_units(units_)), seed(seed_),
        errors(3 * sizeof(unsigned long long), DevBuf::zeroed), block_errors(blocks * sizeof(unsigned), DevBuf::zeroed),
        nrec(sizeof(unsigned), DevBuf::zeroed), recs(CU_CHECK_RECORDS * sizeof(CuCheckRecord), DevBuf::zeroed),
        flip_pos(flip_table(seed_, blocks, units)), loc(blocks * 2 * sizeof(uint32_t), DevBuf::zeroed),
        block_loc(static_cast<size_t>(blocks) * 2) {
    hipDeviceProp_t p;
    AK_HIP(hipGetDeviceProperties(&p, dev));
    if (p.sharedMemPerBlock < static_cast<size_t>(CU_CHECK_LDS_BYTES))
      throw std::runtime_error("cu-check needs 163840 bytes of LDS per workgroup, the device offers " +
                               std::to_string(p.sharedMemPerBlock));
  }
  static int checked_units(int units) {
    if (units < 1 || units > CU_UNIT_ALL) throw std::invalid_argument("units must name at least one of lds, valu, trans");
    return units;
  }
  // Flip i belongs to unit slot i mod n_en; its position is (base + i * stride) mod (blocks * elems) of
  // that unit, elems = 40960 words (lds) or 1024 lanes (valu, trans). The stride is coprime to
  // both moduli (the smaller divides the larger), so the positions of one unit are distinct.
  static std::vector<uint32_t> flip_table(uint32_t seed, int blocks, int units) {
    const unsigned long long small = static_cast<unsigned long long>(blocks) * CU_CHECK_THREADS;
    const unsigned long long large = static_cast<unsigned long long>(blocks) * CU_CHECK_WORDS;
    std::vector<unsigned long long> slot_mod;
    for (int u = 0; u < 3; ++u)
      if (units & (1 << u)) slot_mod.push_back(u == 0 ? large : small);
    return flip_positions(seed, CU_CHECK_MAX_FLIPS, small, large, slot_mod);
  }
  CuCheckArgs args(int rounds, int flips) const {
    CuCheckArgs a = {};
    a.seed = seed;
    a.rounds = rounds;
    a.flips = flips;
    a.units = units;
    a.dbg_block = -1;
    a.flip_pos = flip_pos.as<const uint32_t>();
    a.errors = errors.as<unsigned long long>();
    a.block_errors = block_errors.as<unsigned>();
    a.nrec = nrec.as<unsigned>();
    a.recs = recs.as<CuCheckRecord>();
    a.loc = loc.as<uint32_t>();
    return a;
  }
  void launch(const CuCheckArgs& a) {
    hipLaunchKernelGGL(cu_check_kernel, dim3(blocks), dim3(CU_CHECK_THREADS), 0, 0, a);
    AK_HIP(hipGetLastError());
    ++launches;
  }
  // after a finished launch: where its workgroups ran, and which of them counted errors
  void collect() {
    block_loc = loc.download<uint32_t>();
    const std::vector<unsigned> be = block_errors.download<unsigned>();
    bool any = false;
    for (int b = 0; b < blocks; ++b) {
      const uint32_t key = cu_decode_location(block_loc[2 * b], block_loc[2 * b + 1]).key();
      seen.insert(key);
      if (be[b]) {
        bad[key] += be[b];
        any = true;
      }
    }
    if (any) block_errors.zero();
  }
};

inline CuLocation cu_location_of_key(uint32_t key) {
  CuLocation l;
  l.xcc = key >> 12;
  l.se = (key >> 8) & 15;
  l.sh = (key >> 4) & 15;
  l.cu = key & 15;
  return l;
}

// rounds > 0: one launch of exactly that many rounds. rounds <= 0: calibrated to ~target_ms
// (check_core.h; the self-test flips go into the last launch only).
inline CuCheckResult cu_check_drive(CuCheckRun& run, int rounds, double target_ms, int flips) {
  GpuTimer timer;
  const Calibrated c = calibrate(
      [&](int r, int f) {
        const double ms = timer.time([&] { run.launch(run.args(r, f)); });
        run.collect();
        return ms;
      },
      16, 1 << 26, rounds, target_ms, flips);
  CuCheckResult r;
  const std::vector<unsigned long long> by_unit = run.errors.download<unsigned long long>();
  for (int u = 0; u < 3; ++u) r.errors_by_unit[u] = by_unit[u];
  r.first_errors = fetch_records<CuCheckRecord>(run.nrec, run.recs);
  r.errors = r.errors_by_unit[0] + r.errors_by_unit[1] + r.errors_by_unit[2];
  r.ms = c.ms;
  r.rounds = c.rounds;
  r.blocks = run.blocks;
  r.units = run.units;
  r.launches = run.launches;
  r.cus = run.cus;
  r.cus_covered = static_cast<int>(run.seen.size());
  std::set<int> xccs;
  for (uint32_t key : run.seen) {
    r.locations.push_back(cu_location_of_key(key));
    xccs.insert(static_cast<int>(key >> 12));
  }
  r.xccs = static_cast<int>(xccs.size());
  r.block_loc = run.block_loc;
  for (const auto& kv : run.bad) {
    if (r.bad_cus.size() == static_cast<size_t>(CU_CHECK_RECORDS)) break;
    r.bad_cus.push_back(CuCheckBadCu{cu_location_of_key(kv.first), kv.second});
  }
  // rates of the last launch over its whole time: a unit's own rate when it runs alone
  const double per_s = static_cast<double>(run.blocks) * c.rounds / (c.ms * 1e-3);
  if (run.units & CU_UNIT_LDS) r.lds_gbps = per_s * 6.0 * CU_CHECK_LDS_BYTES / 1e9;  // three store and three load passes
  if (run.units & CU_UNIT_VALU) r.valu_gops = per_s * CU_CHECK_THREADS * CU_CHECK_VALU_MADS / 1e9;
  return r;
}

// Runs the check; while the places seen are fewer than the device's CUs, up to CU_CHECK_EXTRA_LAUNCHES
// further launches of one round each are added (they check as well, and count into errors).
inline CuCheckResult run_cu_check(int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu, int flips = 0,
                                  int units = CU_UNIT_ALL) {
  if (flips < 0 || flips > CU_CHECK_MAX_FLIPS) throw std::invalid_argument("selftest flips must be in [0, 4096]");
  AK_HIP(hipSetDevice(dev));
  CuCheckRun run(dev, seed, units);
  CuCheckResult r = cu_check_drive(run, rounds, target_ms, flips);
  if (r.cus_covered < r.cus) {
    const CuCheckResult first = r;
    for (int i = 0; i < CU_CHECK_EXTRA_LAUNCHES && r.cus_covered < r.cus; ++i) r = cu_check_drive(run, 1, 0, 0);
    r.ms = first.ms;  // the timed launch stays the reported one, with the places of its workgroups
    r.block_loc = first.block_loc;
    r.rounds = first.rounds;
    r.lds_gbps = first.lds_gbps;
    r.valu_gops = first.valu_gops;
  }
  return r;
}

struct CuCheckDump {
  uint32_t hw_id = 0, xcc_id = 0;
  std::vector<uint32_t> lds, valu_ops;
  std::vector<float> valu_f32, trans_in, trans_out;
  std::vector<double> valu_f64;
  std::vector<unsigned long long> valu_int;
};

// one launch of a single round, all units, with workgroup `block` storing its image, operands and results
inline CuCheckDump cu_check_dump_host(int block, uint32_t seed, int dev) {
  AK_HIP(hipSetDevice(dev));
  CuCheckRun run(dev, seed, CU_UNIT_ALL);
  if (block < 0 || block >= run.blocks) throw std::invalid_argument("block out of range");
  const size_t T = CU_CHECK_THREADS;
  DevBuf lds(CU_CHECK_WORDS * 4), ops(T * CU_CHECK_VALU_OPS * 4), f32(T * 4 * 4), f64(T * 3 * 8), i64(T * 4 * 8),
      tin(T * CU_CHECK_TRANS_N * 4), tout(T * CU_CHECK_TRANS_N * 4);
  CuCheckArgs a = run.args(1, 0);
  a.dbg_block = block;
  a.dbg_lds = lds.as<v4u>();
  a.dbg_valu_ops = ops.as<uint32_t>();
  a.dbg_valu_f32 = f32.as<float>();
  a.dbg_valu_f64 = f64.as<double>();
  a.dbg_valu_int = i64.as<unsigned long long>();
  a.dbg_trans_in = tin.as<float>();
  a.dbg_trans_out = tout.as<float>();
  run.launch(a);
  AK_HIP(hipDeviceSynchronize());
  run.collect();
  CuCheckDump d;
  d.hw_id = run.block_loc[2 * block];
  d.xcc_id = run.block_loc[2 * block + 1];
  d.lds = lds.download<uint32_t>();
  d.valu_ops = ops.download<uint32_t>();
  d.valu_f32 = f32.download<float>();
  d.valu_f64 = f64.download<double>();
  d.valu_int = i64.download<unsigned long long>();
  d.trans_in = tin.download<float>();
  d.trans_out = tout.download<float>();
  return d;
}

}  // namespace amdkube
