// The arithmetic of atomic-check: which slot a lane hits in a step and back, the keys, what every op
// adds, and what a slot must hold afterwards. Plain C++17 with no HIP include, so
// native/atomic_plan_selftest.cpp checks it on the CPU, plain and under ASan/UBSan; kernels/atomic_check.h
// runs it on the device (scatter and verify) and on the host (self-test positions). The formulas are
// written out in atomic_check.h; amdkube/ops/atomiccheck.py is written from them.
#pragma once

#include <cstdint>

#include "check_core.h"

namespace amdkube {

constexpr int ATOMIC_WG = 256;                 // lanes of a workgroup
constexpr int ATOMIC_STEPS = 4;                // T: steps of a round
constexpr int ATOMIC_MAX_BLOCKS = 1024;        // G <= 2^18, n = c T <= 2^20: an f64 sum of n 32-bit operands stays below 2^52
constexpr int ATOMIC_PK_BF16_RANKS = 8, ATOMIC_PK_BF16_MAX = 8;    // T * 8 ranks * 8  = 256
constexpr int ATOMIC_PK_F16_RANKS = 16, ATOMIC_PK_F16_MAX = 32;    // T * 16 ranks * 32 = 2048
static_assert(ATOMIC_STEPS * ATOMIC_PK_BF16_RANKS * ATOMIC_PK_BF16_MAX <= 256, "bf16 holds every integer up to 256");
static_assert(ATOMIC_STEPS * ATOMIC_PK_F16_RANKS * ATOMIC_PK_F16_MAX <= 2048, "f16 holds every integer up to 2048");

// op numbers: a record's `op`, a table's index, a name in the dumps
enum : int {
  AOP_ADD_U32, AOP_ADD_U64, AOP_AND, AOP_OR, AOP_XOR, AOP_SMIN, AOP_SMAX, AOP_UMIN, AOP_UMAX, AOP_UMIN_U64, AOP_UMAX_U64,
  AOP_ADD_F32, AOP_ADD_F64, AOP_MIN_F64, AOP_MAX_F64, AOP_PK_ADD_BF16, AOP_PK_ADD_F16, AOP_TICKET, AOP_CAS_ADD, AOP_COUNT
};
constexpr const char* ATOMIC_OP_NAMES[AOP_COUNT] = {"add_u32", "add_u64", "and", "or", "xor", "smin", "smax", "umin", "umax",
                                                    "umin_u64", "umax_u64", "add_f32", "add_f64", "min_f64", "max_f64",
                                                    "pk_add_bf16", "pk_add_f16", "ticket", "cas_add"};
enum : int { ATOMIC_UNIT_INT = 1, ATOMIC_UNIT_FP = 2, ATOMIC_UNIT_RET = 4, ATOMIC_UNIT_LDS = 8, ATOMIC_UNIT_ALL = 15 };
constexpr int ATOMIC_CAS_MAX_CONTENTION = 64;  // the global CAS-loop add runs at c <= 64 only

AK_HOST_DEVICE inline int atomic_op_unit(int op) { return op < AOP_ADD_F32 ? 0 : op < AOP_TICKET ? 1 : 2; }
AK_HOST_DEVICE inline bool atomic_op_is64(int op) {
  return op == AOP_ADD_U64 || op == AOP_UMIN_U64 || op == AOP_UMAX_U64 || (op >= AOP_ADD_F64 && op <= AOP_MAX_F64);
}
// whether the global table of `op` is used at contention c under the units mask
AK_HOST_DEVICE inline bool atomic_op_enabled(int op, int units, uint32_t c) {
  if (!(units & (1 << atomic_op_unit(op)))) return false;
  return op != AOP_CAS_ADD || c <= static_cast<uint32_t>(ATOMIC_CAS_MAX_CONTENTION);
}
// the LDS unit runs every op but the ticket
AK_HOST_DEVICE inline bool atomic_op_in_lds(int op) { return op != AOP_TICKET; }

AK_HOST_DEVICE inline uint32_t atomic_log2(uint32_t pow2) {
  uint32_t l = 0;
  while (l < 31 && (1u << l) < pow2) ++l;
  return l;
}
AK_HOST_DEVICE inline bool atomic_is_pow2(uint32_t x) { return x != 0 && (x & (x - 1)) == 0; }

// The shape of one contention level. G lanes, S = G / c slots, n = c T contributions per slot and round.
struct AtomicShape {
  uint32_t G, c, S, lgS, n;
  uint32_t cl, SL, lgSL, nl;   // the LDS tables of a workgroup: cl = min(c, 256), SL = 256 / cl, nl = cl T
};

AK_HOST_DEVICE inline AtomicShape atomic_shape(uint32_t G, uint32_t c, uint32_t T = ATOMIC_STEPS) {
  AtomicShape s;
  s.G = G;
  s.c = c;
  s.S = G / c;
  s.lgS = atomic_log2(s.S);
  s.n = c * T;
  s.cl = c < static_cast<uint32_t>(ATOMIC_WG) ? c : ATOMIC_WG;
  s.SL = ATOMIC_WG / s.cl;
  s.lgSL = atomic_log2(s.SL);
  s.nl = s.cl * T;
  return s;
}

// The slot map of step `step` of round `round`: p = (g mul + add) & (G - 1), mul odd, so p is a bijection
// of g; slot = p & (S - 1), rank = p >> lgS. inv is mul^-1 mod 2^32 (Newton: x <- x (2 - mul x) doubles the
// correct low bits; x = mul is right to 3 bits, five steps give 96 >= 32).
struct AtomicMap {
  uint32_t mul, add, inv;
};

AK_HOST_DEVICE inline uint32_t atomic_inverse(uint32_t mul) {
  uint32_t x = mul;
  for (int i = 0; i < 5; ++i) x *= 2u - mul * x;
  return x;
}

AK_HOST_DEVICE inline AtomicMap atomic_map(uint32_t seed, uint32_t round, uint32_t step) {
  const uint32_t k = mix32(seed, round, 0x41000000u + step);
  AtomicMap m;
  m.mul = k | 1u;
  m.add = mix32(k ^ 0x85ebca6bu);
  m.inv = atomic_inverse(m.mul);
  return m;
}

AK_HOST_DEVICE inline uint32_t atomic_position(const AtomicMap& m, uint32_t g, uint32_t G) { return (g * m.mul + m.add) & (G - 1); }
AK_HOST_DEVICE inline uint32_t atomic_lane_of(const AtomicMap& m, uint32_t p, uint32_t G) { return ((p - m.add) * m.inv) & (G - 1); }

// the round's operand key, and lane g's value in a step
AK_HOST_DEVICE inline uint32_t atomic_key(uint32_t seed, uint32_t round) { return mix32(seed, round, 0x4b000000u); }
AK_HOST_DEVICE inline uint32_t atomic_value(uint32_t key, uint32_t g, uint32_t step) { return mix32(key, g, step); }

// add_f32 operands are below 2^b with 2^b <= 2^24 / n, so n of them sum to less than 2^24 in any order
AK_HOST_DEVICE inline uint32_t atomic_f32_mask(uint32_t n) {
  const uint32_t lim = (1u << 24) / n;   // n <= 2^20: at least 16
  uint32_t b = 0;
  while ((2u << b) <= lim) ++b;
  return (1u << b) - 1u;
}

// What one contribution adds to each op's slot. v is the lane's value, j its rank at the slot.
struct AtomicOperands {
  uint32_t add_u32, and_, or_, xor_, umin, umax, add_f32, add_f64, pk_bf16, pk_f16, cas;
  int32_t smin, smax, min_f64, max_f64;   // the f64 min and max operands are these integers as doubles
  uint64_t add_u64, umin_u64, umax_u64;
};

AK_HOST_DEVICE inline AtomicOperands atomic_operands(uint32_t v, uint32_t j, uint32_t f32_mask) {
  const uint32_t w = v * 0x85ebca6bu;
  AtomicOperands o;
  o.add_u32 = v;
  o.add_u64 = v * 0x9e3779b97f4a7c15ull;
  o.and_ = ~(1u << (v & 31u));
  o.or_ = 1u << ((v >> 5) & 31u);
  o.xor_ = w;
  o.smin = static_cast<int32_t>(v);
  o.smax = static_cast<int32_t>(w);
  o.umin = w;
  o.umax = v;
  o.umin_u64 = o.add_u64;
  o.umax_u64 = static_cast<uint64_t>(w) << 32 | v;
  o.add_f32 = (v >> 7) & f32_mask;
  o.add_f64 = w;
  o.min_f64 = static_cast<int32_t>(w);
  o.max_f64 = static_cast<int32_t>(v);
  // packed: low half | high half << 16, small integers; past the gate rank both halves are +0
  o.pk_bf16 = j < static_cast<uint32_t>(ATOMIC_PK_BF16_RANKS) ? (1u + (v & 7u)) | (1u + ((v >> 3) & 7u)) << 16 : 0u;
  o.pk_f16 = j < static_cast<uint32_t>(ATOMIC_PK_F16_RANKS) ? (1u + ((v >> 8) & 31u)) | (1u + ((v >> 13) & 31u)) << 16 : 0u;
  o.cas = v ^ 0x5bd1e995u;
  return o;
}

// What a slot must hold, reduced in integers with plain ALU code; every reduction is commutative and
// associative, so parts can be combined in any order (merge).
struct AtomicExpect {
  uint32_t add_u32, and_, or_, xor_, umin, umax, add_f32, pk_bf16, pk_f16, cas;
  int32_t smin, smax, min_f64, max_f64;
  uint64_t add_u64, umin_u64, umax_u64, add_f64;

  AK_HOST_DEVICE void init() {
    add_u32 = or_ = xor_ = umax = add_f32 = pk_bf16 = pk_f16 = cas = 0;
    and_ = umin = 0xffffffffu;
    smin = min_f64 = INT32_MAX;
    smax = max_f64 = INT32_MIN;
    add_u64 = umax_u64 = add_f64 = 0;
    umin_u64 = ~0ull;
  }
  AK_HOST_DEVICE void add(const AtomicOperands& o) {
    add_u32 += o.add_u32;
    add_u64 += o.add_u64;
    and_ &= o.and_;
    or_ |= o.or_;
    xor_ ^= o.xor_;
    smin = o.smin < smin ? o.smin : smin;
    smax = o.smax > smax ? o.smax : smax;
    umin = o.umin < umin ? o.umin : umin;
    umax = o.umax > umax ? o.umax : umax;
    umin_u64 = o.umin_u64 < umin_u64 ? o.umin_u64 : umin_u64;
    umax_u64 = o.umax_u64 > umax_u64 ? o.umax_u64 : umax_u64;
    add_f32 += o.add_f32;
    add_f64 += o.add_f64;
    min_f64 = o.min_f64 < min_f64 ? o.min_f64 : min_f64;
    max_f64 = o.max_f64 > max_f64 ? o.max_f64 : max_f64;
    pk_bf16 += o.pk_bf16;   // the halves stay below 2^16: no carry between them
    pk_f16 += o.pk_f16;
    cas += o.cas;
  }
  AK_HOST_DEVICE void merge(const AtomicExpect& e) {
    add_u32 += e.add_u32;
    add_u64 += e.add_u64;
    and_ &= e.and_;
    or_ |= e.or_;
    xor_ ^= e.xor_;
    smin = e.smin < smin ? e.smin : smin;
    smax = e.smax > smax ? e.smax : smax;
    umin = e.umin < umin ? e.umin : umin;
    umax = e.umax > umax ? e.umax : umax;
    umin_u64 = e.umin_u64 < umin_u64 ? e.umin_u64 : umin_u64;
    umax_u64 = e.umax_u64 > umax_u64 ? e.umax_u64 : umax_u64;
    add_f32 += e.add_f32;
    add_f64 += e.add_f64;
    min_f64 = e.min_f64 < min_f64 ? e.min_f64 : min_f64;
    max_f64 = e.max_f64 > max_f64 ? e.max_f64 : max_f64;
    pk_bf16 += e.pk_bf16;
    pk_f16 += e.pk_f16;
    cas += e.cas;
  }
};

// the bits of an integer x <= 256 as bf16 and of x <= 2048 as f16: both exact, and 0 is +0
AK_HOST_DEVICE inline uint32_t atomic_bf16_bits(uint32_t x) { return __builtin_bit_cast(uint32_t, static_cast<float>(x)) >> 16; }
AK_HOST_DEVICE inline uint32_t atomic_f16_bits(uint32_t x) {
  if (x == 0) return 0;
  uint32_t e = 0;
  while ((2u << e) <= x) ++e;   // 2^e <= x < 2^(e+1), e <= 11
  return (e + 15u) << 10 | ((x << (11 - e)) >> 1 & 0x3ffu);
}

// the word or double word that the table of `op` must hold for the reduction e (the ticket: n)
AK_HOST_DEVICE inline uint64_t atomic_want_bits(const AtomicExpect& e, int op, uint32_t n) {
  switch (op) {
    case AOP_ADD_U32: return e.add_u32;
    case AOP_ADD_U64: return e.add_u64;
    case AOP_AND: return e.and_;
    case AOP_OR: return e.or_;
    case AOP_XOR: return e.xor_;
    case AOP_SMIN: return static_cast<uint32_t>(e.smin);
    case AOP_SMAX: return static_cast<uint32_t>(e.smax);
    case AOP_UMIN: return e.umin;
    case AOP_UMAX: return e.umax;
    case AOP_UMIN_U64: return e.umin_u64;
    case AOP_UMAX_U64: return e.umax_u64;
    case AOP_ADD_F32: return __builtin_bit_cast(uint32_t, static_cast<float>(e.add_f32));
    case AOP_ADD_F64: return __builtin_bit_cast(uint64_t, static_cast<double>(e.add_f64));
    case AOP_MIN_F64: return __builtin_bit_cast(uint64_t, static_cast<double>(e.min_f64));
    case AOP_MAX_F64: return __builtin_bit_cast(uint64_t, static_cast<double>(e.max_f64));
    case AOP_PK_ADD_BF16: return atomic_bf16_bits(e.pk_bf16 & 0xffffu) | atomic_bf16_bits(e.pk_bf16 >> 16) << 16;
    case AOP_PK_ADD_F16: return atomic_f16_bits(e.pk_f16 & 0xffffu) | atomic_f16_bits(e.pk_f16 >> 16) << 16;
    case AOP_TICKET: return n;
    default: return e.cas;
  }
}

// what a slot of the table of `op` holds before a round
AK_HOST_DEVICE inline uint64_t atomic_init_bits(int op) {
  switch (op) {
    case AOP_AND: case AOP_UMIN: return 0xffffffffu;
    case AOP_SMIN: return 0x7fffffffu;
    case AOP_SMAX: return 0x80000000u;
    case AOP_UMIN_U64: return ~0ull;
    case AOP_MIN_F64: return 0x7ff0000000000000ull;   // +inf
    case AOP_MAX_F64: return 0xfff0000000000000ull;   // -inf
    default: return 0;
  }
}

// slot s of a table with `S` slots, all of its contributors of all steps: the verifier's sum, serially
AK_HOST_DEVICE inline AtomicExpect atomic_expect_slot(uint32_t seed, uint32_t round, uint32_t G, uint32_t c, uint32_t s,
                                                      uint32_t T = ATOMIC_STEPS) {
  const AtomicShape sh = atomic_shape(G, c, T);
  const uint32_t key = atomic_key(seed, round), fm = atomic_f32_mask(sh.n);
  AtomicExpect e;
  e.init();
  for (uint32_t i = 0; i < T; ++i) {
    const AtomicMap m = atomic_map(seed, round, i);
    for (uint32_t j = 0; j < c; ++j) {
      const uint32_t g = atomic_lane_of(m, j * sh.S + s, G);
      e.add(atomic_operands(atomic_value(key, g, i), j, fm));
    }
  }
  return e;
}

}  // namespace amdkube
