// Atomic-unit integrity check: a scatter-reduce through the global atomic ALUs (at the L2 and, for device
// scope, on the memory side) and the per-CU LDS atomic ALU whose result is exactly predictable whatever
// the arrival order, verified by a second kernel that uses no atomics on the checked values. Behind
// atomic-check, the device plugin's --atomic-check-ms and hip.atomic_check. The arithmetic (slot map and
// its inverse, keys, operands, expected values) is plain C++ in atomic_plan.h, self-tested on the CPU.
//
// The disciplines of cu_check.h and mfma_check.h hold: every loop is bounded (the CAS loops by
// ATOMIC_CAS_RETRIES), arguments are validated at entry with a uniform return, no workgroup waits on
// another, the units mask and the contention are uniform so every __syncthreads sits in uniform control
// flow, errors are one atomicAdd per lane that saw a mismatch and at most 16 records are kept.
//
// Shape. G = blocks * 256 lanes (blocks a power of two, at most 1024), contention c (a power of two,
// 1 <= c <= G), S = G / c slots per table, T = 4 steps per round, n = c T contributions per slot and round.
//
// Formulas (amdkube/ops/atomiccheck.py is written from these, not from the device):
//   map(r, i)    k = mix32(seed, r, 0x41000000 + i), mul = k | 1, add = mix32(k ^ 0x85ebca6b)
//                lane g, step i of round r: p = (g mul + add) & (G - 1), slot = p & (S - 1), rank j = p >> log2 S.
//                mul is odd, so p is a bijection of g: every slot gets exactly c contributions per step. The
//                verifier walks a slot's contributors as g = ((j S + slot - add) inv) & (G - 1), inv = mul^-1
//                mod 2^32 by Newton iteration.
//   value        key = mix32(seed, r, 0x4b000000), v = mix32(key, g, i), w = v * 0x85ebca6b (mod 2^32)
//   int          add_u32 += v; add_u64 += v * 0x9e3779b97f4a7c15 (mod 2^64); and (from all ones) &= ~(1 << (v & 31));
//                or |= 1 << ((v >> 5) & 31); xor ^= w; smin (from INT_MAX) of int(v); smax (from INT_MIN) of int(w);
//                umin (from all ones) of w; umax of v; umin_u64 (from all ones) of the add_u64 operand;
//                umax_u64 of w << 32 | v
//   fp           add_f32 += float((v >> 7) & (2^b - 1)), 2^b the largest power of two <= 2^24 / n: n operands sum
//                to less than 2^24, so every partial sum in any order is an integer fp32 holds exactly.
//                add_f64 += double(w): n <= 2^20 operands below 2^32 stay below 2^52. min_f64 (from +inf) of
//                double(int(w)); max_f64 (from -inf) of double(int(v)).
//                pk_add_bf16 += (lo, hi) = (1 + (v & 7), 1 + ((v >> 3) & 7)) if j < 8, else (+0, +0);
//                pk_add_f16 += (1 + ((v >> 8) & 31), 1 + ((v >> 13) & 31)) if j < 16, else (+0, +0).
//                The bound: per step at most min(c, 8) contributors of a slot have a rank below 8, each adds at
//                most 8, so a half's sum over the T = 4 steps is at most 4 * 8 * 8 = 256, and bf16 (8 significant
//                bits) holds every integer up to 256; for f16 4 * 16 * 32 = 2048 = 2^11, its 11 significant
//                bits. All addends are non-negative integers, so every partial sum in any order is one of these
//                integers, at every c. The lanes past the gate add +0: they issue the instruction and contend.
//   ret          ticket: old = fetch_add(&ticket[slot], 1); if old < n: order[slot n + old] = i G + g (order starts
//                as 0xffffffff). cas_add += v ^ 0x5bd1e995 as a compare-and-swap loop, at c <= 64 only; a lane's
//                failed attempts are each another lane's success at its slot, at most n - 1 <= 255 in a round, so
//                the bound of 2048 attempts is never reached on a healthy part; a lane that reaches it is an error.
//   lds          every workgroup has tables of SL = 256 / cl slots, cl = min(c, 256): lane t of workgroup b
//                (g = 256 b + t) hits slot p & (SL - 1) with rank p >> log2 SL, p the low 8 bits of the global p,
//                with the same v and the operands above at nl = cl T (the ticket is left out; cas_add is a
//                ds_cmpst loop at every cl, nl - 1 <= 1023 failures at most).
//
// Design. One scatter launch is one round at one contention level: blocks x 256 lanes, each doing T steps of
// up to 19 global atomics to 19 tables at its hashed slot, then T steps of 18 LDS atomics. A table is S
// slots at a pitch of 8 bytes, or of 128 bytes while S <= 4096: the hot slots of a contended table then sit
// in cache lines of their own, and since each op has its own table two ops never share a line either
// (tables start 128-byte aligned). The LDS tables ([19][256] double words, 38 KiB) are initialised by the
// workgroup, hit, and after a __syncthreads verified in the same launch: L = min(cl, 64) lanes share a slot,
// each reduces the contributors of ranks sub, sub + L, ... in registers (AtomicExpect: integers only), an
// xor-butterfly over the L lanes combines the parts with each op's own reduction, and lane sub = 0 compares.
// atomic_verify_kernel does the same for the global tables with L = min(c, 64) lanes per slot, reads the
// tables with plain loads, checks order[slot n .. slot n + n) (every entry an id below T G whose step and lane map
// to the slot; with exactly n writers and the ticket at n the returned values were a permutation of 0..n-1),
// and stores the initial values back. At S = 1 one wave walks all n contributions; the default heavy level
// (c = 4096) keeps that at 64 ranks per lane.
//
// Atomic instructions in the gfx950 disassembly of atomic_scatter_kernel, four of each (one per unrolled
// step; the address is per lane, so none is folded into a wave-uniform form, and none is expanded into a
// compiler-made compare-and-swap loop):
//   add_u32 global_atomic_add, ds_add_u32          add_u64 global_atomic_add_x2, ds_add_u64
//   and     global_atomic_and, ds_and_b32          or      global_atomic_or, ds_or_b32
//   xor     global_atomic_xor, ds_xor_b32          smin    global_atomic_smin, ds_min_i32
//   smax    global_atomic_smax, ds_max_i32         umin    global_atomic_umin, ds_min_u32
//   umax    global_atomic_umax, ds_max_u32         umin_u64 global_atomic_umin_x2, ds_min_u64
//   umax_u64 global_atomic_umax_x2, ds_max_u64     add_f32 global_atomic_add_f32, ds_add_f32
//   add_f64 global_atomic_add_f64, ds_add_f64      min_f64 global_atomic_min_f64, ds_min_f64
//   max_f64 global_atomic_max_f64, ds_max_f64      pk_add_bf16 global_atomic_pk_add_bf16, ds_pk_add_bf16
//   pk_add_f16 global_atomic_pk_add_f16, ds_pk_add_f16
//   ticket  global_atomic_add with the value returned (glc)
//   cas_add global_atomic_cmpswap (returning), ds_cmpst_rtn_b32
// and two global_atomic_add_x2 of the error counters behind branches a healthy part never takes.
#pragma once

#include <cstdlib>
#include <cstring>
#include <memory>

#include "atomic_plan.h"
#include "gpu_common.h"

namespace amdkube {

constexpr int ATOMIC_RECORDS = 16;
constexpr int ATOMIC_MAX_FLIPS = 64;
constexpr int ATOMIC_CAS_RETRIES = 2048;
constexpr uint32_t ATOMIC_HOT_SLOTS = 4096;   // tables of at most this many slots get a 128-byte pitch
constexpr int ATOMIC_DEFAULT_BLOCKS = 512;
constexpr int ATOMIC_LDS_OPS = AOP_COUNT - 1;

// unit: 0 int, 1 fp, 2 ret, 3 lds. Global units: slot is the table slot and offset the byte offset in the
// table of `op` (for an order entry: op = ticket, offset in the order array). lds: slot is
// block * 256 + the LDS slot, offset the byte offset in the LDS table. got and want as two halves each;
// hw_id and xcc_id are the raw words of the wave that compared (for lds: the CU whose LDS ALU it was).
struct AtomicRecord {
  uint32_t unit, op, slot, round, contention, offset, got_lo, got_hi, want_lo, want_hi, hw_id, xcc_id;
};

struct AtomicArgs {
  uint32_t seed, round, G, c;
  int units, dbg_block;
  uint32_t pitch;                 // bytes from slot to slot: 8, or 128 while S <= ATOMIC_HOT_SLOTS
  unsigned long long tbytes;      // bytes from table to table
  unsigned char* tables;          // [AOP_COUNT] tables
  uint32_t* order;                // [G * T]
  unsigned long long* errors;     // [4]: int, fp, ret, lds
  unsigned* nrec;
  AtomicRecord* recs;             // [ATOMIC_RECORDS]
  unsigned long long* dbg_lds;    // [AOP_COUNT][256], dbg_block >= 0: that workgroup's LDS tables before it verifies them
};

inline uint32_t atomic_pitch(uint32_t S) { return S <= ATOMIC_HOT_SLOTS ? 128u : 8u; }
inline unsigned long long atomic_table_bytes(uint32_t S) {
  return (static_cast<unsigned long long>(S) * atomic_pitch(S) + 127ull) & ~127ull;
}

// uniform: a launch with arguments that do not fit together does nothing
__device__ __forceinline__ bool atomic_args_ok(const AtomicArgs& a) {
  return atomic_is_pow2(a.G) && a.G >= ATOMIC_WG && a.G <= ATOMIC_MAX_BLOCKS * ATOMIC_WG && atomic_is_pow2(a.c) && a.c <= a.G &&
         a.units >= 1 && a.units <= ATOMIC_UNIT_ALL && (a.pitch == 8u || a.pitch == 128u) &&
         a.tbytes >= static_cast<unsigned long long>(a.G / a.c) * a.pitch;
}

__device__ __noinline__ void atomic_store_record(unsigned* nrec, AtomicRecord* recs, uint32_t unit_op, uint32_t slot,
                                                 uint32_t round, uint32_t contention, uint32_t offset, uint64_t got,
                                                 uint64_t want) {
  const unsigned at = atomicAdd(nrec, 1u);
  if (at < ATOMIC_RECORDS)
    recs[at] = AtomicRecord{unit_op >> 8, unit_op & 255u, slot, round, contention, offset, static_cast<uint32_t>(got),
                            static_cast<uint32_t>(got >> 32), static_cast<uint32_t>(want), static_cast<uint32_t>(want >> 32),
                            __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID), __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID)};
}

typedef __bf16 atomic_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 atomic_f16x2 __attribute__((ext_vector_type(2)));

// One contribution to every enabled op: `at(op)` is the slot's address in the table of op. kLds picks the
// scope (workgroup, on LDS) and the packed builtins of the LDS ALU.
template <bool kLds, class At>
__device__ __forceinline__ void atomic_issue(At&& at, const AtomicOperands& o, bool do_int, bool do_fp) {
  constexpr int scope = kLds ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  if (do_int) {
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(at(AOP_ADD_U32)), o.add_u32, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(at(AOP_ADD_U64)), static_cast<unsigned long long>(o.add_u64),
                           __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_and(reinterpret_cast<uint32_t*>(at(AOP_AND)), o.and_, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_or(reinterpret_cast<uint32_t*>(at(AOP_OR)), o.or_, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_xor(reinterpret_cast<uint32_t*>(at(AOP_XOR)), o.xor_, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_min(reinterpret_cast<int32_t*>(at(AOP_SMIN)), o.smin, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_max(reinterpret_cast<int32_t*>(at(AOP_SMAX)), o.smax, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_min(reinterpret_cast<uint32_t*>(at(AOP_UMIN)), o.umin, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_max(reinterpret_cast<uint32_t*>(at(AOP_UMAX)), o.umax, __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_min(reinterpret_cast<unsigned long long*>(at(AOP_UMIN_U64)), static_cast<unsigned long long>(o.umin_u64),
                           __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_max(reinterpret_cast<unsigned long long*>(at(AOP_UMAX_U64)), static_cast<unsigned long long>(o.umax_u64),
                           __ATOMIC_RELAXED, scope);
  }
  if (do_fp) {
    __hip_atomic_fetch_add(reinterpret_cast<float*>(at(AOP_ADD_F32)), static_cast<float>(o.add_f32), __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_add(reinterpret_cast<double*>(at(AOP_ADD_F64)), static_cast<double>(o.add_f64), __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_min(reinterpret_cast<double*>(at(AOP_MIN_F64)), static_cast<double>(o.min_f64), __ATOMIC_RELAXED, scope);
    __hip_atomic_fetch_max(reinterpret_cast<double*>(at(AOP_MAX_F64)), static_cast<double>(o.max_f64), __ATOMIC_RELAXED, scope);
    // small integers as bf16 / f16 bit patterns, the low half in the low 16 bits
    const uint32_t bf = atomic_bf16_bits(o.pk_bf16 & 0xffffu) | atomic_bf16_bits(o.pk_bf16 >> 16) << 16;
    const uint32_t hf = atomic_f16_bits(o.pk_f16 & 0xffffu) | atomic_f16_bits(o.pk_f16 >> 16) << 16;
    if (kLds) {
      __builtin_amdgcn_ds_atomic_fadd_v2bf16(reinterpret_cast<atomic_bf16x2*>(at(AOP_PK_ADD_BF16)),
                                             __builtin_bit_cast(atomic_bf16x2, bf));
      __builtin_amdgcn_ds_atomic_fadd_v2f16(reinterpret_cast<atomic_f16x2*>(at(AOP_PK_ADD_F16)),
                                            __builtin_bit_cast(atomic_f16x2, hf));
    } else {
      __builtin_amdgcn_global_atomic_fadd_v2bf16(reinterpret_cast<atomic_bf16x2*>(at(AOP_PK_ADD_BF16)),
                                                 __builtin_bit_cast(atomic_bf16x2, bf));
      __builtin_amdgcn_global_atomic_fadd_v2f16(reinterpret_cast<atomic_f16x2*>(at(AOP_PK_ADD_F16)),
                                                __builtin_bit_cast(atomic_f16x2, hf));
    }
  }
}

// *p += x as a compare-and-swap loop of at most ATOMIC_CAS_RETRIES attempts; false: the lane ran out
template <bool kLds>
__device__ __forceinline__ bool atomic_cas_add(uint32_t* p, uint32_t x) {
  constexpr int scope = kLds ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  uint32_t old = __hip_atomic_load(p, __ATOMIC_RELAXED, scope);
  for (int tries = 0; tries < ATOMIC_CAS_RETRIES; ++tries)
    if (__hip_atomic_compare_exchange_strong(p, &old, old + x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, scope)) return true;
  return false;
}

__device__ __forceinline__ AtomicExpect atomic_shfl_xor(const AtomicExpect& e, int m) {
  AtomicExpect o;
  o.add_u32 = __shfl_xor(e.add_u32, m);
  o.and_ = __shfl_xor(e.and_, m);
  o.or_ = __shfl_xor(e.or_, m);
  o.xor_ = __shfl_xor(e.xor_, m);
  o.umin = __shfl_xor(e.umin, m);
  o.umax = __shfl_xor(e.umax, m);
  o.add_f32 = __shfl_xor(e.add_f32, m);
  o.pk_bf16 = __shfl_xor(e.pk_bf16, m);
  o.pk_f16 = __shfl_xor(e.pk_f16, m);
  o.cas = __shfl_xor(e.cas, m);
  o.smin = __shfl_xor(e.smin, m);
  o.smax = __shfl_xor(e.smax, m);
  o.min_f64 = __shfl_xor(e.min_f64, m);
  o.max_f64 = __shfl_xor(e.max_f64, m);
  o.add_u64 = __shfl_xor(static_cast<unsigned long long>(e.add_u64), m);
  o.umin_u64 = __shfl_xor(static_cast<unsigned long long>(e.umin_u64), m);
  o.umax_u64 = __shfl_xor(static_cast<unsigned long long>(e.umax_u64), m);
  o.add_f64 = __shfl_xor(static_cast<unsigned long long>(e.add_f64), m);
  return o;
}

// What slot `s` of a table with 2^lgS slots must hold, worked out by the L lanes (a power of two <= 64,
// consecutive in a wave) that share it: lane `sub` reduces the contributors of ranks sub, sub + L, ... < c
// of every step, the butterfly combines the parts. Contributor (rank j, step i) is lane
// gbase + (((j 2^lgS + s - add_i) inv_i) & (N - 1)) of the grid. Every lane of the wave calls this (idle
// lanes with active = false): the shuffles sit in uniform control flow.
__device__ __forceinline__ AtomicExpect atomic_expect(const AtomicMap (&maps)[ATOMIC_STEPS], uint32_t key, uint32_t gbase,
                                                      uint32_t N, uint32_t lgS, uint32_t c, uint32_t s, uint32_t sub, uint32_t L,
                                                      uint32_t f32_mask, bool active) {
  AtomicExpect e;
  e.init();
  for (uint32_t j = active ? sub : c; j < c; j += L) {   // at most c / L ranks
#pragma unroll
    for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) {
      const uint32_t g = gbase + atomic_lane_of(maps[i], (j << lgS) + s, N);
      e.add(atomic_operands(atomic_value(key, g, i), j, f32_mask));
    }
  }
  for (uint32_t m = 1; m < L; m <<= 1) e.merge(atomic_shfl_xor(e, static_cast<int>(m)));   // at most 6 stages
  return e;
}

// Compares the slot at `at(op)` of every op that `enabled(op)` names with the reduction e and stores the
// initial value back. Returns the mismatches; bit u of *units_bad says that unit u had one.
template <class At, class Enabled>
__device__ __forceinline__ unsigned atomic_compare(At&& at, Enabled&& enabled, const AtomicExpect& e, uint32_t n,
                                                   const AtomicArgs& a, int lds_unit, uint32_t slot, uint32_t offset,
                                                   unsigned* bad_by_unit) {
  unsigned bad = 0;
#pragma unroll
  for (int op = 0; op < AOP_COUNT; ++op) {
    if (!enabled(op)) continue;
    unsigned char* p = at(op);
    const uint64_t got = atomic_op_is64(op) ? *reinterpret_cast<const unsigned long long*>(p) : *reinterpret_cast<const uint32_t*>(p);
    const uint64_t want = atomic_want_bits(e, op, n);
    if (got != want) {
      const int unit = lds_unit >= 0 ? lds_unit : atomic_op_unit(op);
      ++bad;
      ++bad_by_unit[unit];
      atomic_store_record(a.nrec, a.recs, static_cast<uint32_t>(unit) << 8 | op, slot, a.round, a.c, offset, got, want);
    }
    if (atomic_op_is64(op))
      *reinterpret_cast<unsigned long long*>(p) = atomic_init_bits(op);
    else
      *reinterpret_cast<uint32_t*>(p) = static_cast<uint32_t>(atomic_init_bits(op));
  }
  return bad;
}

// ---------------------------------------------------------------------------- kernels
// every slot of every table to its initial value, every order entry to 0xffffffff: G lanes
__global__ __launch_bounds__(ATOMIC_WG) void atomic_init_kernel(AtomicArgs a) {
  if (!atomic_args_ok(a) || gridDim.x * ATOMIC_WG != a.G) return;
  const uint32_t g = blockIdx.x * ATOMIC_WG + threadIdx.x, S = a.G / a.c;
  if (g < S) {
#pragma unroll
    for (int op = 0; op < AOP_COUNT; ++op)
      *reinterpret_cast<unsigned long long*>(a.tables + op * a.tbytes + static_cast<size_t>(g) * a.pitch) = atomic_init_bits(op);
  }
#pragma unroll
  for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) a.order[g * ATOMIC_STEPS + i] = 0xffffffffu;
}

// the hot one: one round at one contention level
__global__ __launch_bounds__(ATOMIC_WG) void atomic_scatter_kernel(AtomicArgs a) {
  __shared__ unsigned long long lds[AOP_COUNT][ATOMIC_WG];
  if (!atomic_args_ok(a) || gridDim.x * ATOMIC_WG != a.G) return;
  const AtomicShape sh = atomic_shape(a.G, a.c);
  const uint32_t t = threadIdx.x, g = blockIdx.x * ATOMIC_WG + t;
  const uint32_t key = atomic_key(a.seed, a.round);
  const bool do_int = a.units & ATOMIC_UNIT_INT, do_fp = a.units & ATOMIC_UNIT_FP, do_ret = a.units & ATOMIC_UNIT_RET;
  const bool do_lds = a.units & ATOMIC_UNIT_LDS, do_cas = do_ret && a.c <= ATOMIC_CAS_MAX_CONTENTION;
  AtomicMap maps[ATOMIC_STEPS];
#pragma unroll
  for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) maps[i] = atomic_map(a.seed, a.round, i);
  unsigned ran_out = 0, ran_out_lds = 0;

  if (do_int || do_fp || do_ret) {
    const uint32_t fm = atomic_f32_mask(sh.n);
#pragma unroll
    for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) {
      const uint32_t p = atomic_position(maps[i], g, a.G), s = p & (sh.S - 1), j = p >> sh.lgS;
      const AtomicOperands o = atomic_operands(atomic_value(key, g, i), j, fm);
      unsigned char* base = a.tables + static_cast<size_t>(s) * a.pitch;
      auto at = [&](int op) { return base + op * a.tbytes; };
      atomic_issue<false>(at, o, do_int, do_fp);
      if (do_ret) {
        const uint32_t old = __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(at(AOP_TICKET)), 1u, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
        if (old < sh.n) a.order[s * sh.n + old] = i * a.G + g;   // s n + old < S n = G T
      }
      if (do_cas && !atomic_cas_add<false>(reinterpret_cast<uint32_t*>(at(AOP_CAS_ADD)), o.cas)) ++ran_out;
    }
  }

  if (do_lds) {   // uniform
#pragma unroll
    for (int op = 0; op < AOP_COUNT; ++op) lds[op][t] = atomic_init_bits(op);
    __syncthreads();
    const uint32_t fm = atomic_f32_mask(sh.nl);
#pragma unroll
    for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) {
      const uint32_t p = atomic_position(maps[i], g, ATOMIC_WG), s = p & (sh.SL - 1), j = p >> sh.lgSL;
      const AtomicOperands o = atomic_operands(atomic_value(key, g, i), j, fm);
      auto at = [&](int op) { return reinterpret_cast<unsigned char*>(&lds[op][s]); };
      atomic_issue<true>(at, o, true, true);
      if (!atomic_cas_add<true>(reinterpret_cast<uint32_t*>(at(AOP_CAS_ADD)), o.cas)) ++ran_out_lds;
    }
    __syncthreads();
    if (static_cast<int>(blockIdx.x) == a.dbg_block) {
#pragma unroll
      for (int op = 0; op < AOP_COUNT; ++op) a.dbg_lds[op * ATOMIC_WG + t] = lds[op][t];
      __syncthreads();   // uniform: a whole workgroup dumps or none of it
    }
    // L lanes to a slot: lane t has slot t / L and part t % L; SL L <= 256, the lanes past it idle
    const uint32_t L = sh.cl < 64u ? sh.cl : 64u, lgL = atomic_log2(L);
    const uint32_t s = t >> lgL, sub = t & (L - 1);
    const bool active = s < sh.SL;
    const AtomicExpect e = atomic_expect(maps, key, blockIdx.x * ATOMIC_WG, ATOMIC_WG, sh.lgSL, sh.cl, active ? s : 0u, sub, L, fm,
                                         active);
    if (active && sub == 0) {
      unsigned by_unit[4] = {0, 0, 0, 0};
      auto at = [&](int op) { return reinterpret_cast<unsigned char*>(&lds[op][s]); };
      atomic_compare(at, [](int op) { return atomic_op_in_lds(op); }, e, sh.nl, a, 3, blockIdx.x * ATOMIC_WG + s, s * 8u, by_unit);
      ran_out_lds += by_unit[3];
    }
  }
  if (ran_out) atomicAdd(a.errors + 2, static_cast<unsigned long long>(ran_out));   // none on a healthy part
  if (ran_out_lds) atomicAdd(a.errors + 3, static_cast<unsigned long long>(ran_out_lds));
}

// the self-test: one bit of `nflips` table slots, flips[2 k] the op and flips[2 k + 1] the slot
__global__ __launch_bounds__(ATOMIC_WG) void atomic_flip_kernel(AtomicArgs a, const uint32_t* flips, int nflips) {
  if (!atomic_args_ok(a) || nflips < 0 || nflips > ATOMIC_MAX_FLIPS) return;
  const int k = blockIdx.x * ATOMIC_WG + threadIdx.x;
  if (k >= nflips) return;
  const uint32_t op = flips[2 * k], s = flips[2 * k + 1];
  if (op >= AOP_COUNT || s >= a.G / a.c) return;
  *reinterpret_cast<uint32_t*>(a.tables + op * a.tbytes + static_cast<size_t>(s) * a.pitch) ^= 1u;
}

// S * min(c, 64) lanes: recompute, compare with plain loads, re-initialise
__global__ __launch_bounds__(ATOMIC_WG) void atomic_verify_kernel(AtomicArgs a) {
  if (!atomic_args_ok(a)) return;
  const AtomicShape sh = atomic_shape(a.G, a.c);
  const uint32_t L = a.c < 64u ? a.c : 64u, lgL = atomic_log2(L);
  if (static_cast<unsigned long long>(gridDim.x) * ATOMIC_WG < static_cast<unsigned long long>(sh.S) * L) return;
  const uint32_t gid = blockIdx.x * ATOMIC_WG + threadIdx.x, s = gid >> lgL, sub = gid & (L - 1);
  const bool active = s < sh.S;
  const uint32_t key = atomic_key(a.seed, a.round), fm = atomic_f32_mask(sh.n);
  AtomicMap maps[ATOMIC_STEPS];
#pragma unroll
  for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) maps[i] = atomic_map(a.seed, a.round, i);
  const AtomicExpect e = atomic_expect(maps, key, 0u, a.G, sh.lgS, a.c, active ? s : 0u, sub, L, fm, active);
  unsigned by_unit[4] = {0, 0, 0, 0};
  if (active && sub == 0) {
    unsigned char* base = a.tables + static_cast<size_t>(s) * a.pitch;
    auto at = [&](int op) { return base + op * a.tbytes; };
    atomic_compare(at, [&](int op) { return atomic_op_enabled(op, a.units, a.c); }, e, sh.n, a, -1, s, s * a.pitch, by_unit);
  }
  if (active && (a.units & ATOMIC_UNIT_RET)) {
    // this lane's share of the slot's order entries: those of its ranks
    const uint32_t lgG = atomic_log2(a.G);
    for (uint32_t j = sub; j < a.c; j += L) {
#pragma unroll
      for (uint32_t i = 0; i < ATOMIC_STEPS; ++i) {
        const uint32_t at = s * sh.n + j * ATOMIC_STEPS + i, id = a.order[at];
        const uint32_t step = id >> lgG, lane = id & (a.G - 1);
        bool ok = step < ATOMIC_STEPS;
        if (ok) {
          AtomicMap m = maps[0];
#pragma unroll
          for (uint32_t q = 1; q < ATOMIC_STEPS; ++q)
            if (step == q) m = maps[q];
          ok = (atomic_position(m, lane, a.G) & (sh.S - 1)) == s;
        }
        if (!ok) {
          ++by_unit[2];
          atomic_store_record(a.nrec, a.recs, 2u << 8 | AOP_TICKET, s, a.round, a.c, at * 4u, id, 0xffffffffu);
        }
        a.order[at] = 0xffffffffu;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (by_unit[u]) atomicAdd(a.errors + u, static_cast<unsigned long long>(by_unit[u]));   // none on a healthy part
}

// ---------------------------------------------------------------------------- runners
constexpr const char* ATOMIC_UNIT_NAMES[4] = {"int", "fp", "ret", "lds"};

// c = 1 spreads over every slot and so every L2 channel, 64 is one wave's worth on a slot, 4096 is heavy
inline std::vector<uint32_t> atomic_default_contention() { return {1u, 64u, 4096u}; }

// "1,64,4096" -> the levels; throws std::invalid_argument unless every one is a power of two in [1, 2^18]
inline std::vector<uint32_t> atomic_check_contention(const std::string& list) {
  std::vector<uint32_t> out;
  for (const std::string& name : split_list(list)) {
    char* end = nullptr;
    const unsigned long v = std::strtoul(name.c_str(), &end, 10);
    if (name.empty() || *end || v > static_cast<unsigned long>(ATOMIC_MAX_BLOCKS * ATOMIC_WG) || !atomic_is_pow2(static_cast<uint32_t>(v)))
      throw std::invalid_argument("contention '" + name + "': expected a comma list of powers of two in [1, 262144]");
    out.push_back(static_cast<uint32_t>(v));
  }
  return out;
}

inline int atomic_global_ops(int units, uint32_t c) {
  int n = 0;
  for (int op = 0; op < AOP_COUNT; ++op) n += atomic_op_enabled(op, units, c);
  return n;
}

// slot-ops that one round checks at contention c, and the atomic instructions it issues (a CAS loop is one)
inline unsigned long long atomic_checked_per_round(int blocks, uint32_t c, int units) {
  const AtomicShape sh = atomic_shape(static_cast<uint32_t>(blocks) * ATOMIC_WG, c);
  return static_cast<unsigned long long>(sh.S) * atomic_global_ops(units, c) +
         (units & ATOMIC_UNIT_LDS ? static_cast<unsigned long long>(blocks) * sh.SL * ATOMIC_LDS_OPS : 0ull);
}
inline unsigned long long atomic_issued_per_round(int blocks, uint32_t c, int units) {
  return static_cast<unsigned long long>(blocks) * ATOMIC_WG * ATOMIC_STEPS *
         (atomic_global_ops(units, c) + (units & ATOMIC_UNIT_LDS ? ATOMIC_LDS_OPS : 0));
}

struct AtomicFlip {
  uint32_t op, slot, contention;
};

struct AtomicCheckResult {
  double ms = 0, atomics_per_s = 0;
  long long rounds = 0;
  int blocks = 0, units = 0;
  std::vector<uint32_t> contention;
  unsigned long long checked = 0, errors = 0, errors_by_unit[4] = {0, 0, 0, 0};
  std::vector<AtomicFlip> flipped;
  std::vector<AtomicRecord> first_errors;
};

// the tables of one contention level, initialised by atomic_init_kernel
struct AtomicLevel {
  AtomicShape sh;
  int blocks;
  DevBuf tables, order;
  AtomicLevel(int blocks_, uint32_t c)
      : sh(atomic_shape(static_cast<uint32_t>(blocks_) * ATOMIC_WG, c)), blocks(blocks_),
        tables(AOP_COUNT * atomic_table_bytes(sh.S)), order(static_cast<size_t>(sh.G) * ATOMIC_STEPS * sizeof(uint32_t)) {}
};

struct AtomicCheckRun {
  int blocks, units;
  uint32_t seed;
  std::vector<std::unique_ptr<AtomicLevel>> levels;
  DevBuf errors, nrec, recs, flips;
  AtomicCheckRun(int blocks_, uint32_t seed_, int units_, const std::vector<uint32_t>& contention)
      : blocks(blocks_), units(units_), seed(seed_), errors(4 * sizeof(unsigned long long), DevBuf::zeroed),
        nrec(sizeof(unsigned), DevBuf::zeroed), recs(ATOMIC_RECORDS * sizeof(AtomicRecord), DevBuf::zeroed),
        flips(2 * ATOMIC_MAX_FLIPS * sizeof(uint32_t), DevBuf::zeroed) {
    if (blocks < 1 || blocks > ATOMIC_MAX_BLOCKS || !atomic_is_pow2(static_cast<uint32_t>(blocks)))
      throw std::invalid_argument("blocks must be a power of two in [1, 1024]");
    if (units < 1 || units > ATOMIC_UNIT_ALL) throw std::invalid_argument("units must name at least one of int, fp, ret, lds");
    if (contention.empty()) throw std::invalid_argument("the contention list is empty");
    for (uint32_t c : contention) {
      if (!atomic_is_pow2(c) || c > static_cast<uint32_t>(blocks) * ATOMIC_WG)
        throw std::invalid_argument("contention " + std::to_string(c) + " is not a power of two in [1, " +
                                    std::to_string(blocks * ATOMIC_WG) + "] (the lanes of " + std::to_string(blocks) + " workgroups)");
    }
    for (uint32_t c : contention) {
      levels.push_back(std::make_unique<AtomicLevel>(blocks, c));
      hipLaunchKernelGGL(atomic_init_kernel, dim3(blocks), dim3(ATOMIC_WG), 0, 0, args(*levels.back(), 0));
      AK_HIP(hipGetLastError());
    }
  }
  AtomicArgs args(const AtomicLevel& l, uint32_t round) const {
    AtomicArgs a = {};
    a.seed = seed;
    a.round = round;
    a.G = l.sh.G;
    a.c = l.sh.c;
    a.units = units;
    a.dbg_block = -1;
    a.pitch = atomic_pitch(l.sh.S);
    a.tbytes = atomic_table_bytes(l.sh.S);
    a.tables = l.tables.as<unsigned char>();
    a.order = l.order.as<uint32_t>();
    a.errors = errors.as<unsigned long long>();
    a.nrec = nrec.as<unsigned>();
    a.recs = recs.as<AtomicRecord>();
    return a;
  }
  void scatter(const AtomicArgs& a) {
    hipLaunchKernelGGL(atomic_scatter_kernel, dim3(blocks), dim3(ATOMIC_WG), 0, 0, a);
    AK_HIP(hipGetLastError());
  }
  void verify(const AtomicLevel& l, const AtomicArgs& a) {
    const unsigned long long lanes = static_cast<unsigned long long>(l.sh.S) * (l.sh.c < 64u ? l.sh.c : 64u);   // <= G
    hipLaunchKernelGGL(atomic_verify_kernel, dim3(static_cast<unsigned>((lanes + ATOMIC_WG - 1) / ATOMIC_WG)), dim3(ATOMIC_WG), 0, 0, a);
    AK_HIP(hipGetLastError());
  }
  // The self-test's positions at the first level: flip k sits at position q_k of flip_positions (check_core.h)
  // over ops * S, op = the (q_k mod ops)-th enabled global op, slot = q_k / ops. Distinct while n <= ops * S.
  std::vector<AtomicFlip> plan_flips(int n) const {
    const AtomicLevel& l = *levels.front();
    std::vector<uint32_t> ops;
    for (int op = 0; op < AOP_COUNT; ++op)
      if (atomic_op_enabled(op, units, l.sh.c)) ops.push_back(static_cast<uint32_t>(op));
    const unsigned long long positions = ops.size() * static_cast<unsigned long long>(l.sh.S);
    if (static_cast<unsigned long long>(n) > positions)
      throw std::invalid_argument("selftest flips need a global unit (int, fp, ret) and at most one flip per table slot of the first level");
    std::vector<AtomicFlip> out;
    for (uint32_t q : flip_positions(seed, static_cast<size_t>(n), positions))
      out.push_back(AtomicFlip{ops[q % ops.size()], static_cast<uint32_t>(q / ops.size()), l.sh.c});
    return out;
  }
  void flip(const AtomicLevel& l, const AtomicArgs& a, const std::vector<AtomicFlip>& f) {
    std::vector<uint32_t> words;
    for (const AtomicFlip& x : f) {
      words.push_back(x.op);
      words.push_back(x.slot);
    }
    AK_HIP(hipMemcpy(flips.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(atomic_flip_kernel, dim3(1), dim3(ATOMIC_WG), 0, 0, a, flips.as<const uint32_t>(), static_cast<int>(f.size()));
    AK_HIP(hipGetLastError());
    (void)l;
  }
};

// rounds > 0: exactly that many rounds. rounds <= 0: calibrated to ~target_ms (check_core.h; the self-test
// flips go into round 0 of the last timed run, at the first contention level). A round is, per contention
// level, a scatter launch and a verify launch on the one stream.
inline AtomicCheckResult run_atomic_check(int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu, int flips = 0,
                                          int units = ATOMIC_UNIT_ALL, std::vector<uint32_t> contention = {},
                                          int blocks = ATOMIC_DEFAULT_BLOCKS) {
  if (flips < 0 || flips > ATOMIC_MAX_FLIPS) throw std::invalid_argument("selftest flips must be in [0, 64]");
  if (contention.empty()) contention = atomic_default_contention();
  AK_HIP(hipSetDevice(dev));
  AtomicCheckRun run(blocks, seed, units, contention);
  AtomicCheckResult r;
  r.flipped = run.plan_flips(flips);
  GpuTimer timer;
  long long total_rounds = 0;
  const Calibrated c = calibrate(
      [&](int n, int f) {
        total_rounds += n;
        return timer.time([&] {
          for (int round = 0; round < n; ++round)
            for (size_t li = 0; li < run.levels.size(); ++li) {
              const AtomicLevel& l = *run.levels[li];
              const AtomicArgs a = run.args(l, static_cast<uint32_t>(round));
              run.scatter(a);
              if (f > 0 && round == 0 && li == 0) run.flip(l, a, r.flipped);
              run.verify(l, a);
            }
        });
      },
      2, 1 << 16, rounds, target_ms, flips);
  fetch_outcome(r, c, run.errors, run.nrec, run.recs);
  r.blocks = blocks;
  r.units = units;
  r.contention = contention;
  unsigned long long issued = 0;
  for (uint32_t cc : contention) {
    r.checked += atomic_checked_per_round(blocks, cc, units) * static_cast<unsigned long long>(total_rounds);
    issued += atomic_issued_per_round(blocks, cc, units);
  }
  r.atomics_per_s = c.ms > 0 ? static_cast<double>(issued) * c.rounds / (c.ms * 1e-3) : 0;   // of the last timed run
  return r;
}

struct AtomicTables {
  AtomicShape sh;
  std::vector<std::vector<unsigned long long>> table;   // [AOP_COUNT][S]: the slots, 32-bit ops zero-extended
  std::vector<uint32_t> order;                          // [G * T]
  std::vector<std::vector<unsigned long long>> lds;     // [AOP_COUNT][SL] of workgroup 0
};

// init and one scatter launch of round `round`; nothing verifies or re-initialises (tests only)
inline AtomicTables atomic_check_tables_host(uint32_t contention, int blocks, uint32_t seed, uint32_t round, int units, int dev) {
  AK_HIP(hipSetDevice(dev));
  AtomicCheckRun run(blocks, seed, units, {contention});
  const AtomicLevel& l = *run.levels.front();
  DevBuf dbg(AOP_COUNT * ATOMIC_WG * sizeof(unsigned long long), DevBuf::zeroed);
  AtomicArgs a = run.args(l, round);
  a.dbg_block = 0;
  a.dbg_lds = dbg.as<unsigned long long>();
  run.scatter(a);
  AK_HIP(hipDeviceSynchronize());
  AtomicTables out;
  out.sh = l.sh;
  const std::vector<unsigned char> raw = l.tables.download<unsigned char>();
  const std::vector<unsigned long long> lds = dbg.download<unsigned long long>();
  out.table.resize(AOP_COUNT);
  out.lds.resize(AOP_COUNT);
  for (int op = 0; op < AOP_COUNT; ++op) {
    for (uint32_t s = 0; s < l.sh.S; ++s) {
      unsigned long long v = 0;
      std::memcpy(&v, raw.data() + op * a.tbytes + static_cast<size_t>(s) * a.pitch, atomic_op_is64(op) ? 8 : 4);
      out.table[op].push_back(v);
    }
    for (uint32_t s = 0; s < l.sh.SL; ++s) out.lds[op].push_back(atomic_op_is64(op) ? lds[op * ATOMIC_WG + s] : lds[op * ATOMIC_WG + s] & 0xffffffffull);
  }
  out.order = l.order.download<uint32_t>();
  return out;
}

}  // namespace amdkube
