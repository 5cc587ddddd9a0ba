// Lane check: the hardware that moves data between lanes and into LDS without going through a lane's own
// registers. Behind lane-check, the device plugin's --lane-check-ms and hip.lane_check. Four units behind the
// `units` mask, each verified bit for bit in the same launch, every round:
//   dpp   the VALU cross-lane network: 40 DPP controls (lane_plan.h: quad_perm, row_shl/shr/ror, row_mirror,
//         row_half_mirror, row_bcast:15/31, wave_shl/rol/shr/ror, each keeping old and zero-filling, a partial
//         row mask and a partial bank mask), v_permlane16_swap_b32 and v_permlane32_swap_b32 on both returned
//         registers, v_readlane_b32 at a lane taken from the key
//   perm  the LDS crossbar as a permute unit: ds_bpermute_b32 with a hashed pull map (duplicates), ds_permute_b32
//         with a hashed bijection, ds_swizzle_b32 in quad-perm and bit-mask mode
//   tr    the transposing LDS reads ds_read_b64_tr_b16 / _b8 / _b4 and ds_read_b96_tr_b6 on a tile that
//         plain ds_write stored, the lanes' rows 24 or 48 bytes apart
//   dma   global_load_lds_dword / _dwordx3 / _dwordx4 sweeping the whole 160 KiB of LDS from a source buffer
//         that a launch of its own filled, read back with plain ds_read_b128
// The operations are pure permutations: lane t of the workgroup holds v = mix32(key + t), so the exact result
// is mix32(key + source), the source worked out in integer arithmetic on the lane id by lane_plan.h. The
// expected value needs no data movement and shares nothing with the unit under test.
//
// Every cross-lane instruction is issued with the full EXEC mask in uniform control flow: the units mask,
// the round and the template flags are uniform, the kernel is launched with whole waves only, and a lane that
// sees a mismatch leaves the straight path only after the instruction, for an out-of-line record.
//
// The disciplines of cu_check.h hold. A workgroup has 1024 threads and declares all 163,840 B of LDS, so it
// owns its CU; the grid is 4 workgroups per CU. Every loop is bounded, arguments are validated at entry with
// a uniform return, there is no synchronisation between workgroups, every barrier sits in uniform control
// flow, errors are one atomicAdd per lane that saw a mismatch, at most 16 records are kept. Every wave
// stores its raw HW_ID (the cross-lane network belongs to a SIMD), wave 0 the XCC_ID.
//
// Formulas (amdkube/ops/lanecheck.py is written from these and lane_plan.h, not from the device):
//   key(tag, r)  = mix32(seed, block, tag + r): lane_key, tags 0x44 dpp, 0x50 perm, 0x58 + form tr (top byte)
//   dpp, perm    v(t) = mix32(key + t), old(t) = mix32((key ^ 0x5bd1e995) + t), t the lane of the workgroup;
//                a result whose source is lane s of the wave is v(64 wave + s). The swaps run on (A, B) = (v, old).
//                bpermute pulls from mix32((key ^ 0x5bd1e995) + t) & 63.
//   tr           element E = wave * 64 * per_row + e of form f is the low bits of mix32(key + E)
//   dma          src[i] = mix32(mix32(seed ^ 0x646d6121) + i), LDS word w of workgroup b from i = 40960 b + w;
//                the LDS holds 0xdeadbeef ^ round before the sweep
// Observed on an MI355X (lane_plan.h has the formulas): the swaps and every DPP control, permute and swizzle
// do what the ISA text says. The transposing reads hand lane l' of a 16-lane block M[k j + l' div per_row]
// [l' mod per_row], not the map first expected. global_load_lds_dwordx3 strides the lanes by 16 bytes in LDS,
// not 12, and writes three words of each slot; M0 reaches all 160 KiB. The immediate offset moves the global
// address as well as the LDS address.
#pragma once

#include <utility>

#include "cu_run.h"
#include "gpu_common.h"
#include "lane_plan.h"

namespace amdkube {

constexpr int LANE_SLOTS_PER_LANE = LANE_WORDS / 4 / LANE_THREADS;  // 10 16-byte slots
constexpr int LANE_BLOCKS_PER_CU = 4;
constexpr int LANE_RECORDS = 16;
constexpr int LANE_MAX_FLIPS = 4096;
constexpr int LANE_EXTRA_LAUNCHES = 3;  // added one by one while a run has not seen every SIMD
constexpr int LANE_LOC_WORDS = LANE_WAVES + 1;  // per workgroup: the HW_ID of each wave, then XCC_ID
constexpr int LANE_SRC_PAD = 1024;              // words past the last image of the dma source
constexpr int LANE_TR_BYTES_PER_LANE = 8 + 8 + 8 + 12;
enum : int { LANE_UNIT_DPP = 1, LANE_UNIT_PERM = 2, LANE_UNIT_TR = 4, LANE_UNIT_DMA = 8, LANE_UNIT_ALL = 15 };

typedef __attribute__((address_space(3))) char* lane_lds_ptr;
typedef __attribute__((address_space(1))) void* lane_global_ptr;
typedef short lane_v4s __attribute__((ext_vector_type(4)));
typedef int lane_v2i __attribute__((ext_vector_type(2)));
typedef int lane_v3i __attribute__((ext_vector_type(3)));

// unit: 0 dpp, 1 perm, 2 tr, 3 dma. dpp, perm: op is the column of the result table, lane the lane of the
// workgroup. tr: op is 4 form + register. dma: op is the width mode of the region (0 dword, 1 dwordx3,
// 2 dwordx4) and lane the LDS word. hw_id and xcc_id are the raw words of the wave that saw the mismatch.
struct LaneCheckRecord {
  uint32_t unit, block, round, op, lane, got, want, hw_id, xcc_id;
};

struct LaneCheckArgs {
  uint32_t seed;
  int rounds, flips, units, dbg_block;
  const uint32_t* flip_pos;            // LANE_MAX_FLIPS positions, see LaneCheckRun
  const uint32_t* src;                 // [blocks * LANE_WORDS + LANE_SRC_PAD], the dma source
  unsigned long long* errors;          // [4]: dpp, perm, tr, dma
  unsigned* block_errors;              // [blocks]
  unsigned* nrec;
  LaneCheckRecord* recs;               // [LANE_RECORDS]
  uint32_t* loc;                       // [blocks][LANE_LOC_WORDS]
  // dbg_block >= 0: that workgroup also stores, in round 0 (tests only)
  uint32_t* dbg_dpp;                   // [1024][LANE_DPP_OPS]
  uint32_t* dbg_perm;                  // [1024][LANE_PERM_OPS]
  uint32_t* dbg_tr;                    // [1024][9]: b16 0 1, b8 0 1, b4 0 1, b6 0 1 2
  v4u* dbg_dma;                        // [10240] the image after the sweep
};

struct LaneCtx {
  const LaneCheckArgs* a;
  int round;
  unsigned mine;     // record slots this lane has asked for
  int flip_op;       // self-test: the op of this lane whose compared copy gets flip_bit, or -1
  uint32_t flip_bit;
  uint32_t* dbg;     // this lane's row of the unit's result table, or nullptr
};

// out of line and by value, as in cu_check.h: the mismatch path must not cost the straight path registers
__device__ __noinline__ void lane_check_store_record(unsigned* nrec, LaneCheckRecord* recs, uint32_t unit_op, uint32_t round,
                                                     uint32_t lane, uint32_t got, uint32_t want) {
  const unsigned slot = atomicAdd(nrec, 1u);
  if (slot < LANE_RECORDS)
    recs[slot] = LaneCheckRecord{unit_op >> 16, blockIdx.x, round, unit_op & 0xffffu, lane, got, want,
                                 __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID), __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID)};
}

// compares one result word (after the dump and the self-test flip); returns the mismatches, 0 or 1
__device__ __forceinline__ unsigned lane_compare(LaneCtx& cx, uint32_t unit, int op, uint32_t lane, uint32_t got, uint32_t want) {
  if (cx.dbg) cx.dbg[op] = got;
  if (cx.flip_op == op) got ^= cx.flip_bit;
  __builtin_amdgcn_sched_barrier(0);  // one op at a time: the expected values are not all hashed ahead of their compares
  if (got == want) return 0;
  if (cx.mine < LANE_RECORDS) {  // a lane asks for at most 16 slots however long it runs
    ++cx.mine;
    lane_check_store_record(cx.a->nrec, cx.a->recs, unit << 16 | static_cast<uint32_t>(op), static_cast<uint32_t>(cx.round), lane,
                            got, want);
  }
  return 1;
}

// Self-test flips of `round` that belong to the unit in slot `us` of the `n_en` enabled units: flip i goes
// to unit slot i mod n_en and round (i / n_en) mod rounds, at position p = flip_pos[i] = block * elems +
// element (distinct positions, chosen by the host). hit(element, p). At most LANE_MAX_FLIPS iterations.
template <class F>
__device__ __forceinline__ void lane_check_flips(const LaneCheckArgs& a, int round, int us, int n_en, uint32_t elems, F&& hit) {
  for (int q = round; q * n_en + us < a.flips; q += a.rounds) {
    const uint32_t p = a.flip_pos[q * n_en + us], b = p / elems;
    if (b == blockIdx.x) hit(p - b * elems, p);
  }
}

// dpp, perm, tr: the element is the lane of the workgroup, the op mix32(p) mod ops, the bit (mix32(p) >> 16) & 31
template <bool kFlip>
__device__ __forceinline__ void lane_flip_of_lane(LaneCtx& cx, int us, int n_en, int ops) {
  cx.flip_op = -1;
  cx.flip_bit = 0;
  if (kFlip)
    lane_check_flips(*cx.a, cx.round, us, n_en, LANE_THREADS, [&](uint32_t lane, uint32_t p) {
      if (lane == threadIdx.x) {
        cx.flip_op = static_cast<int>(mix32(p) % static_cast<uint32_t>(ops));
        cx.flip_bit = 1u << ((mix32(p) >> 16) & 31u);
      }
    });
}

// The lane id of this round: what it was, but the compiler no longer knows it. The source lanes do not depend on
// the round, and hoisted out of the round loop they would all stay in registers and spill.
__device__ __forceinline__ uint32_t lane_id_of_round() {
  uint32_t t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// ---------------------------------------------------------------------------- dpp
// the value that source s (lane_plan.h) stands for, in the wave whose first lane is wb
__device__ __forceinline__ uint32_t lane_value_of(int s, uint32_t key, uint32_t wb, uint32_t old) {
  return s >= 0 ? mix32(key + wb + static_cast<uint32_t>(s)) : s == LANE_SRC_ZERO ? 0u : old;
}

template <int I>
__device__ __forceinline__ unsigned lane_dpp_one(LaneCtx& cx, uint32_t t, uint32_t key, uint32_t v, uint32_t old) {
  constexpr LaneDpp d = lane_dpp(I);
  const uint32_t got = __builtin_amdgcn_update_dpp(old, v, d.ctrl, d.row_mask, d.bank_mask, d.bound_ctrl);
  return lane_compare(cx, 0, I, t, got, lane_value_of(lane_dpp_src(d, static_cast<int>(t & 63u)), key, t & ~63u, old));
}

template <size_t... I>
__device__ __forceinline__ unsigned lane_dpp_round(LaneCtx& cx, std::index_sequence<I...>) {
  const LaneCheckArgs& a = *cx.a;
  const uint32_t t = lane_id_of_round(), wb = t & ~63u;
  const int l = static_cast<int>(t & 63u);
  const uint32_t key = lane_key(a.seed, blockIdx.x, LANE_TAG_DPP, cx.round), ko = key ^ LANE_OLD_XOR;
  // old is never zero-folded: with old = 0 the compiler turns the move into its bound_ctrl form
  const uint32_t v = mix32(key + t), old = mix32(ko + t);
  unsigned bad = (lane_dpp_one<static_cast<int>(I)>(cx, t, key, v, old) + ... + 0u);
  auto swapped = [&](int width, int reg) {
    const LaneSwapSrc s = lane_swap_src(width, reg, l);
    return mix32((s.reg ? ko : key) + wb + static_cast<uint32_t>(s.lane));
  };
  const auto s16 = __builtin_amdgcn_permlane16_swap(v, old, false, false);
  bad += lane_compare(cx, 0, LANE_OP_SWAP16, t, s16[0], swapped(16, 0));
  bad += lane_compare(cx, 0, LANE_OP_SWAP16 + 1, t, s16[1], swapped(16, 1));
  const auto s32 = __builtin_amdgcn_permlane32_swap(v, old, false, false);
  bad += lane_compare(cx, 0, LANE_OP_SWAP32, t, s32[0], swapped(32, 0));
  bad += lane_compare(cx, 0, LANE_OP_SWAP32 + 1, t, s32[1], swapped(32, 1));
  const int idx = __builtin_amdgcn_readfirstlane(lane_readlane_index(key, static_cast<int>(t >> 6)));
  bad += lane_compare(cx, 0, LANE_OP_READLANE, t, __builtin_amdgcn_readlane(v, idx), mix32(key + wb + static_cast<uint32_t>(idx)));
  return bad;
}

// ---------------------------------------------------------------------------- perm
template <int I>
__device__ __forceinline__ unsigned lane_swizzle_one(LaneCtx& cx, uint32_t t, uint32_t key, uint32_t v) {
  constexpr int offset = LANE_SWIZZLE[I];
  const uint32_t got = __builtin_amdgcn_ds_swizzle(v, offset);
  return lane_compare(cx, 1, LANE_OP_SWIZZLE + I, t, got, mix32(key + (t & ~63u) + lane_swizzle_src(offset, static_cast<int>(t & 63u))));
}

template <size_t... I>
__device__ __forceinline__ unsigned lane_perm_round(LaneCtx& cx, std::index_sequence<I...>) {
  const LaneCheckArgs& a = *cx.a;
  const uint32_t t = lane_id_of_round(), wb = t & ~63u;
  const int l = static_cast<int>(t & 63u), wave = static_cast<int>(t >> 6);
  const uint32_t key = lane_key(a.seed, blockIdx.x, LANE_TAG_PERM, cx.round);
  const uint32_t v = mix32(key + t);
  unsigned bad = 0;
  const int pull = lane_bpermute_src(key ^ LANE_OLD_XOR, static_cast<int>(t));
  bad += lane_compare(cx, 1, LANE_OP_BPERMUTE, t, __builtin_amdgcn_ds_bpermute(4 * pull, v), mix32(key + wb + static_cast<uint32_t>(pull)));
  const int pa = lane_permute_a(key, wave), pb = lane_permute_b(key, wave);
  bad += lane_compare(cx, 1, LANE_OP_PERMUTE, t, __builtin_amdgcn_ds_permute(4 * lane_permute_dst(pa, pb, l), v),
                      mix32(key + wb + static_cast<uint32_t>(lane_permute_src(pa, pb, l))));
  bad += (lane_swizzle_one<static_cast<int>(I)>(cx, t, key, v) + ... + 0u);
  return bad;
}

// ---------------------------------------------------------------------------- tr
// the row or result register set of `kForm` packed from the elements elem(0 .. per_row - 1), little-endian
template <int kForm, class E>
__device__ __forceinline__ void lane_tr_pack(uint32_t (&w)[3], uint32_t key, E&& elem) {
  constexpr int bits = LANE_TR_BITS[kForm], per = LANE_TR_PER_LANE[kForm];
  w[0] = w[1] = w[2] = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    const uint32_t x = mix32(key + elem(j)) & ((1u << bits) - 1u);
    const int at = j * bits, word = at >> 5, shift = at & 31;
    w[word] |= x << shift;
    if (shift + bits > 32) w[word + 1] |= x >> (32 - shift);
  }
}

// One form: the wave stores its tile with plain ds_write, one row a lane, reads it back transposed and compares
// every register with the word packed from the elements lane_tr_element names.
template <int kForm>
__device__ __forceinline__ unsigned lane_tr_form(lane_lds_ptr lds, LaneCtx& cx) {
  constexpr int per = LANE_TR_PER_LANE[kForm], regs = LANE_TR_REGS[kForm];
  constexpr int first_reg = kForm == LANE_TR_B6 ? 6 : 2 * kForm;
  const LaneCheckArgs& a = *cx.a;
  const uint32_t t = lane_id_of_round(), wave = t >> 6;
  const int l = static_cast<int>(t & 63u);
  const uint32_t key = lane_key(a.seed, blockIdx.x, LANE_TAG_TR + (static_cast<uint32_t>(kForm) << 24), cx.round);
  const uint32_t tile = wave * 64u * per;  // the wave's first element
  lane_lds_ptr row = lds + wave * LANE_TR_SLICE + l * LANE_TR_STRIDE[kForm];
  uint32_t w[3];
  lane_tr_pack<kForm>(w, key, [&](int j) { return tile + static_cast<uint32_t>(l * per + j); });
#pragma unroll
  for (int r = 0; r < regs; ++r) reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(row)[r] = w[r];
  __syncthreads();
  uint32_t got[3] = {0, 0, 0};
  if constexpr (kForm == LANE_TR_B16) {
    const lane_v4s x = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) lane_v4s*>(row));
    got[0] = static_cast<uint16_t>(x.x) | static_cast<uint32_t>(static_cast<uint16_t>(x.y)) << 16;
    got[1] = static_cast<uint16_t>(x.z) | static_cast<uint32_t>(static_cast<uint16_t>(x.w)) << 16;
  } else if constexpr (kForm == LANE_TR_B8) {
    const lane_v2i x = __builtin_amdgcn_ds_read_tr8_b64_v2i32(reinterpret_cast<__attribute__((address_space(3))) lane_v2i*>(row));
    got[0] = x.x, got[1] = x.y;
  } else if constexpr (kForm == LANE_TR_B4) {
    const lane_v2i x = __builtin_amdgcn_ds_read_tr4_b64_v2i32(reinterpret_cast<__attribute__((address_space(3))) lane_v2i*>(row));
    got[0] = x.x, got[1] = x.y;
  } else {
    const lane_v3i x = __builtin_amdgcn_ds_read_tr6_b96_v3i32(reinterpret_cast<__attribute__((address_space(3))) lane_v3i*>(row));
    got[0] = x.x, got[1] = x.y, got[2] = x.z;
  }
  lane_tr_pack<kForm>(w, key, [&](int j) { return tile + static_cast<uint32_t>(lane_tr_element(kForm, l, j)); });
  unsigned bad = 0;
#pragma unroll
  for (int r = 0; r < regs; ++r) {
    if (cx.dbg) cx.dbg[first_reg + r] = got[r];
    uint32_t g = got[r];
    if (cx.flip_op == kForm && r == 0) g ^= cx.flip_bit;
    if (g != w[r]) {
      ++bad;
      if (cx.mine < LANE_RECORDS) {
        ++cx.mine;
        lane_check_store_record(a.nrec, a.recs, 2u << 16 | static_cast<uint32_t>(4 * kForm + r), static_cast<uint32_t>(cx.round), t, g,
                                w[r]);
      }
    }
  }
  __syncthreads();  // the slice is free for the next form or unit
  return bad;
}

// ---------------------------------------------------------------------------- dma
// One direct load of W bytes a lane with the immediate offset IMM: the LDS base goes to M0 and is the same for
// the whole wave, the global address is the lane's own. Both are lowered by IMM, which the instruction adds back.
template <int W, int IMM>
__device__ __forceinline__ void lane_dma_issue(const uint32_t* g_region, lane_lds_ptr l_region, int word, int l) {
  const char* g = reinterpret_cast<const char*>(g_region + word) + lane_dma_lane_offset(W, l) - IMM;
  const lane_global_ptr gp = (lane_global_ptr)g;  // address-space casts: C style only
  const lane_lds_ptr lp = l_region + (4 * word - IMM);
  // the builtin checks its size while the template is still being read, so it wants the literal
  if constexpr (W == 4)
    __builtin_amdgcn_global_load_lds(gp, lp, 4, IMM, 0);
  else if constexpr (W == 12)
    __builtin_amdgcn_global_load_lds(gp, lp, 12, IMM, 0);
  else
    __builtin_amdgcn_global_load_lds(gp, lp, 16, IMM, 0);
}

// the chunks of lane_dma_chunk(M, .) in order; the one with the immediate offset is peeled, the rest is a loop
// (unrolled in full, the sweep keeps an address pair a chunk in registers and spills)
template <int M>
__device__ __forceinline__ void lane_dma_sweep(const uint32_t* g_region, lane_lds_ptr l_region, int l) {
  constexpr int W = lane_dma_chunk(M, 0).width;
  static_assert(LANE_DMA_IMM_CHUNK == 1 && lane_dma_chunk(M, 0).imm == 0 && lane_dma_chunk(M, 1).imm == LANE_DMA_IMM &&
                lane_dma_chunk(M, 2).imm == 0, "the peeled chunk is chunk 1");
  lane_dma_issue<W, 0>(g_region, l_region, lane_dma_chunk(M, 0).word, l);
  lane_dma_issue<W, LANE_DMA_IMM>(g_region, l_region, lane_dma_chunk(M, 1).word, l);
#pragma unroll 2
  for (int i = 2; i < lane_dma_chunks(M); ++i) lane_dma_issue<W, 0>(g_region, l_region, lane_dma_chunk(M, i).word, l);
}

template <bool kFlip>
__device__ __forceinline__ unsigned long long lane_dma_flip_mask(LaneCtx& cx, int us, int n_en) {
  unsigned long long m = 0;
  if (kFlip)
    lane_check_flips(*cx.a, cx.round, us, n_en, LANE_WORDS, [&](uint32_t word, uint32_t) {
      const uint32_t slot = word >> 2;
      if ((slot & (LANE_THREADS - 1)) == threadIdx.x) m |= 1ull << (4 * (slot / LANE_THREADS) + (word & 3u));
    });
  return m;
}

// One round: clear the LDS, sweep it with the direct loads of this round's widths, wait, compare it all.
// fm: self-test mask over the lane's 40 compared words (bit 4 j + c), XORed into the compared copy only.
template <bool kFlip>
__device__ __forceinline__ unsigned lane_dma_round(v4u* img, lane_lds_ptr lds, LaneCtx& cx, unsigned long long fm, bool dbg) {
  const LaneCheckArgs& a = *cx.a;
  const uint32_t t = threadIdx.x;
  const int l = static_cast<int>(t & 63u);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(t >> 6));  // the LDS base is wave-uniform: say so
  const uint32_t clear = LANE_DMA_CLEAR ^ static_cast<uint32_t>(cx.round);
#pragma unroll
  for (int j = 0; j < LANE_SLOTS_PER_LANE; ++j) img[j * LANE_THREADS + t] = v4u{clear, clear, clear, clear};
  __syncthreads();
  const uint32_t* g_region = a.src + static_cast<size_t>(blockIdx.x) * LANE_WORDS + wave * LANE_DMA_REGION;
  lane_lds_ptr l_region = lds + 4 * wave * LANE_DMA_REGION;
  const int mode = lane_dma_mode(wave, cx.round);
  if (mode == 0)  // uniform within the wave
    lane_dma_sweep<0>(g_region, l_region, l);
  else if (mode == 1)
    lane_dma_sweep<1>(g_region, l_region, l);
  else
    lane_dma_sweep<2>(g_region, l_region, l);
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0): the loads have landed in LDS
  __syncthreads();
  const uint32_t skey = lane_dma_source_key(a.seed) + blockIdx.x * static_cast<uint32_t>(LANE_WORDS);
  unsigned bad = 0;
#pragma unroll 2
  for (int j = 0; j < LANE_SLOTS_PER_LANE; ++j) {
    const uint32_t slot = j * LANE_THREADS + t, w0 = 4u * slot;
    const int m = lane_dma_mode(static_cast<int>(w0 / LANE_DMA_REGION), cx.round);
    v4u got = img[slot];
    if (dbg && cx.round == 0) a.dbg_dma[slot] = got;
    const v4u want = v4u{mix32(skey + w0), mix32(skey + w0 + 1u), mix32(skey + w0 + 2u), m == 1 ? clear : mix32(skey + w0 + 3u)};
    if (kFlip) {
      const uint32_t f = static_cast<uint32_t>(fm >> (4 * j)) & 15u;
      got ^= v4u{f & 1u, (f >> 1) & 1u, (f >> 2) & 1u, (f >> 3) & 1u};
    }
    const v4u d = got ^ want;
    if ((d.x | d.y | d.z | d.w) != 0) {  // the healthy path: one branch per slot
#pragma unroll 1
      for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t g = c == 0 ? got.x : c == 1 ? got.y : c == 2 ? got.z : got.w;
        const uint32_t e = c == 0 ? want.x : c == 1 ? want.y : c == 2 ? want.z : want.w;
        if (g != e) {
          ++bad;
          if (cx.mine < LANE_RECORDS) {
            ++cx.mine;
            lane_check_store_record(a.nrec, a.recs, 3u << 16 | static_cast<uint32_t>(m), static_cast<uint32_t>(cx.round), w0 + c, g, e);
          }
        }
      }
    }
  }
  __syncthreads();  // the image is free for the next round
  return bad;
}

// the source of the direct loads: src[i] = mix32(skey + i); a launch of its own, once per run
__global__ __launch_bounds__(256) void lane_dma_fill_kernel(uint32_t* src, size_t n, uint32_t skey) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    src[i] = mix32(skey + static_cast<uint32_t>(i));
}

// ---------------------------------------------------------------------------- the kernel
// kFlip: the self-test is on; kDbg: some workgroup dumps (never both: the dump launch has no flips)
template <bool kFlip, bool kDbg>
__device__ __forceinline__ void lane_check_body(v4u* img, const LaneCheckArgs& a) {
  const bool dbg = kDbg && static_cast<int>(blockIdx.x) == a.dbg_block;
  const lane_lds_ptr lds = (lane_lds_ptr)img;  // address-space casts: C style only
  const int n_en = __builtin_popcount(static_cast<unsigned>(a.units));
  auto slot_of = [&](int unit) { return __builtin_popcount(static_cast<unsigned>(a.units) & (static_cast<unsigned>(unit) - 1u)); };
  LaneCtx cx{&a, 0, 0, -1, 0, nullptr};
  unsigned bad[4] = {0, 0, 0, 0};
  for (int round = 0; round < a.rounds; ++round) {
    cx.round = round;
    const bool dump = dbg && round == 0;
    if (a.units & LANE_UNIT_DPP) {
      lane_flip_of_lane<kFlip>(cx, slot_of(LANE_UNIT_DPP), n_en, LANE_DPP_OPS);
      cx.dbg = dump ? a.dbg_dpp + threadIdx.x * LANE_DPP_OPS : nullptr;
      bad[0] += lane_dpp_round(cx, std::make_index_sequence<LANE_DPP_N>());
    }
    if (a.units & LANE_UNIT_PERM) {
      lane_flip_of_lane<kFlip>(cx, slot_of(LANE_UNIT_PERM), n_en, LANE_PERM_OPS);
      cx.dbg = dump ? a.dbg_perm + threadIdx.x * LANE_PERM_OPS : nullptr;
      bad[1] += lane_perm_round(cx, std::make_index_sequence<LANE_SWIZZLE_N>());
    }
    if (a.units & LANE_UNIT_TR) {
      lane_flip_of_lane<kFlip>(cx, slot_of(LANE_UNIT_TR), n_en, LANE_TR_FORMS);
      cx.dbg = dump ? a.dbg_tr + threadIdx.x * LANE_TR_REG_TOTAL : nullptr;
      bad[2] += lane_tr_form<LANE_TR_B16>(lds, cx) + lane_tr_form<LANE_TR_B8>(lds, cx) + lane_tr_form<LANE_TR_B4>(lds, cx) +
                lane_tr_form<LANE_TR_B6>(lds, cx);
    }
    if (a.units & LANE_UNIT_DMA)
      bad[3] += lane_dma_round<kFlip>(img, lds, cx, lane_dma_flip_mask<kFlip>(cx, slot_of(LANE_UNIT_DMA), n_en), dbg);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (bad[u]) {  // one per lane that saw a mismatch: none on a healthy part
      atomicAdd(a.errors + u, static_cast<unsigned long long>(bad[u]));
      atomicAdd(a.block_errors + blockIdx.x, bad[u]);
    }
}

__global__ __launch_bounds__(LANE_THREADS) void lane_check_kernel(LaneCheckArgs a) {
  __shared__ __attribute__((aligned(16))) v4u img[LANE_WORDS / 4];
  // uniform: never index past the flip table, never loop on a non-positive stride, whole waves only
  if (a.rounds < 1 || a.flips < 0 || a.flips > LANE_MAX_FLIPS || a.units < 1 || a.units > LANE_UNIT_ALL ||
      blockDim.x != LANE_THREADS)
    return;
  if ((threadIdx.x & 63u) == 0) {  // every wave reads its place once
    a.loc[LANE_LOC_WORDS * blockIdx.x + (threadIdx.x >> 6)] = __builtin_amdgcn_s_getreg(CU_HWREG_HW_ID);
    if (threadIdx.x == 0) a.loc[LANE_LOC_WORDS * blockIdx.x + LANE_WAVES] = __builtin_amdgcn_s_getreg(CU_HWREG_XCC_ID);
  }
  if (a.flips > 0)
    lane_check_body<true, false>(img, a);
  else if (a.dbg_block >= 0)
    lane_check_body<false, true>(img, a);
  else
    lane_check_body<false, false>(img, a);
}

// ---------------------------------------------------------------------------- runners
static_assert(LANE_LDS_BYTES == CU_RUN_LDS_BYTES && LANE_BLOCKS_PER_CU == CU_RUN_BLOCKS_PER_CU && LANE_RECORDS == CU_RUN_RECORDS,
              "the kernel is launched and read back by cu_run.h");

// unit u has the mask bit 1 << u and the number u in a record
constexpr const char* LANE_UNIT_NAMES[4] = {"dpp", "perm", "tr", "dma"};
constexpr unsigned long long LANE_UNIT_ELEMS[4] = {LANE_THREADS, LANE_THREADS, LANE_THREADS, LANE_WORDS};

struct LaneCheckResult : CuRunResult<LaneCheckRecord, 4> {
  double xlane_gops = 0, tr_gbps = 0, dma_gbps = 0;
  int simds = 0, simds_covered = 0;
};

// block_loc is [blocks][LANE_LOC_WORDS]; src is the dma unit's source
struct LaneCheckRun : CuRun {
  DevBuf src;
  LaneCheckRun(int dev, uint32_t seed_, int units_)
      : CuRun("lane-check", dev, seed_, units_, LANE_UNIT_NAMES, 4, sizeof(LaneCheckRecord), LANE_WAVES, flip_table),
        src(units & LANE_UNIT_DMA ? source_words() * sizeof(uint32_t) : 0) {
    if (units & LANE_UNIT_DMA) {  // a launch of its own: the check relies on no visibility between workgroups
      hipLaunchKernelGGL(lane_dma_fill_kernel, dim3(blocks), dim3(256), 0, 0, src.as<uint32_t>(), source_words(),
                         lane_dma_source_key(seed));
      AK_HIP(hipGetLastError());
      AK_HIP(hipDeviceSynchronize());
    }
  }
  size_t source_words() const { return static_cast<size_t>(blocks) * LANE_WORDS + LANE_SRC_PAD; }
  // Flip i belongs to unit slot i mod n_en; its position is (base + i * stride) mod (blocks * elems) of that
  // unit, elems = 1024 lanes (dpp, perm, tr) or 40960 words (dma): check_core.h keeps them distinct.
  static std::vector<uint32_t> flip_table(uint32_t seed, int blocks, int units) {
    std::vector<unsigned long long> slot_mod;
    for (int u = 0; u < 4; ++u)
      if (units & (1 << u)) slot_mod.push_back(static_cast<unsigned long long>(blocks) * LANE_UNIT_ELEMS[u]);
    return flip_positions(seed, LANE_MAX_FLIPS, static_cast<unsigned long long>(blocks) * LANE_THREADS,
                          static_cast<unsigned long long>(blocks) * LANE_WORDS, slot_mod);
  }
  LaneCheckArgs args(int rounds, int flips) const {
    LaneCheckArgs a = CuRun::args<LaneCheckArgs>(rounds, flips);
    a.src = src.as<const uint32_t>();
    return a;
  }
  void launch(const LaneCheckArgs& a) { CuRun::launch(lane_check_kernel, LANE_THREADS, a); }
  bool covered() const { return coverage.simds_covered() >= 4 * cus; }
  // rates of the timed launch over its whole time: a unit's own rate when it runs alone
  void finish(LaneCheckResult& r, const Calibrated& c) const {
    r.simds = 4 * cus;
    r.simds_covered = coverage.simds_covered();
    const double per_s = static_cast<double>(blocks) * c.rounds / (c.ms * 1e-3);
    const int xlane_ops = (units & LANE_UNIT_DPP ? LANE_DPP_OPS : 0) + (units & LANE_UNIT_PERM ? LANE_PERM_OPS : 0);
    r.xlane_gops = per_s * LANE_THREADS * xlane_ops / 1e9;
    if (units & LANE_UNIT_TR) r.tr_gbps = per_s * LANE_THREADS * LANE_TR_BYTES_PER_LANE / 1e9;
    if (units & LANE_UNIT_DMA) r.dma_gbps = per_s * (LANE_DMA_BYTES_3_ROUNDS / 3.0) / 1e9;  // bytes landed in LDS
  }
};

// Runs the check (cu_run.h); while the SIMDs seen are fewer than four to a CU, up to LANE_EXTRA_LAUNCHES
// further launches of one round each are added.
inline LaneCheckResult run_lane_check(int rounds, double target_ms, int dev, uint32_t seed = 0x5eedu, int flips = 0,
                                      int units = LANE_UNIT_ALL) {
  if (flips < 0 || flips > LANE_MAX_FLIPS) throw std::invalid_argument("selftest flips must be in [0, 4096]");
  AK_HIP(hipSetDevice(dev));
  LaneCheckRun run(dev, seed, units);
  return cu_run<LaneCheckResult>(run, rounds, target_ms, flips, LANE_EXTRA_LAUNCHES);
}

struct LaneCheckDump {
  std::vector<uint32_t> dpp, perm, tr, dma, hw_id;
  uint32_t xcc_id = 0;
};

// one launch of a single round, all units, with workgroup `block` storing its result tables and LDS image
inline LaneCheckDump lane_check_dump_host(int block, uint32_t seed, int dev) {
  AK_HIP(hipSetDevice(dev));
  LaneCheckRun run(dev, seed, LANE_UNIT_ALL);
  if (block < 0 || block >= run.blocks) throw std::invalid_argument("block out of range");
  const size_t T = LANE_THREADS;
  DevBuf dpp(T * LANE_DPP_OPS * 4), perm(T * LANE_PERM_OPS * 4), tr(T * LANE_TR_REG_TOTAL * 4), dma(LANE_WORDS * 4);
  LaneCheckArgs a = run.args(1, 0);
  a.dbg_block = block;
  a.dbg_dpp = dpp.as<uint32_t>();
  a.dbg_perm = perm.as<uint32_t>();
  a.dbg_tr = tr.as<uint32_t>();
  a.dbg_dma = dma.as<v4u>();
  run.launch(a);
  AK_HIP(hipDeviceSynchronize());
  run.collect();
  LaneCheckDump d;
  d.dpp = dpp.download<uint32_t>();
  d.perm = perm.download<uint32_t>();
  d.tr = tr.download<uint32_t>();
  d.dma = dma.download<uint32_t>();
  const uint32_t* w = &run.block_loc[static_cast<size_t>(block) * LANE_LOC_WORDS];
  d.hw_id.assign(w, w + LANE_WAVES);
  d.xcc_id = w[LANE_WAVES];
  return d;
}

}  // namespace amdkube
