// The plan of the lane check (lane_check.h): which lane, LDS element or LDS word every result of the
// cross-lane, transposing-read and direct-to-LDS instructions comes from. Plain C++ (constexpr, host and
// device): the kernel computes its expected values from these functions, amdkube/ops/lanecheck.py is
// written from the same formulas, and native/lane_plan_selftest.cpp checks them on the CPU against naive
// loops (ranges, bijections, permutations, and that the dma sweep writes every LDS word exactly once but
// for the fourth word of the dwordx3 slots, which no direct load writes).
#pragma once

#include "check_core.h"

namespace amdkube {

constexpr int LANE_LDS_BYTES = 163840;
constexpr int LANE_WORDS = LANE_LDS_BYTES / 4;  // 40,960
constexpr int LANE_THREADS = 1024;
constexpr int LANE_WAVES = LANE_THREADS / 64;   // 16

// a result comes from lane `src` >= 0 of the same wave, or is zero, or keeps the destination's old value
constexpr int LANE_SRC_ZERO = -1, LANE_SRC_OLD = -2;

// ---------------------------------------------------------------------------- dpp
// DPP control words of gfx9: quad_perm 0x00-0xff (two bits per lane of the quad), row_shl:n 0x100 + n,
// row_shr:n 0x110 + n, row_ror:n 0x120 + n, wave_shl:1 0x130, wave_rol:1 0x134, wave_shr:1 0x138,
// wave_ror:1 0x13c, row_mirror 0x140, row_half_mirror 0x141, row_bcast:15 0x142, row_bcast:31 0x143.
struct LaneDpp {
  int ctrl, row_mask, bank_mask;
  bool bound_ctrl;
};

constexpr int LANE_DPP_QUAD_A = 0x1b;  // quad_perm:[3,2,1,0]
constexpr int LANE_DPP_QUAD_B = 0x4e;  // quad_perm:[2,3,0,1]
constexpr int LANE_DPP_BASE = 19;
// every control once; row_bcast:15 and row_bcast:31 with the row masks of a wave reduction (0xa, 0xc)
constexpr LaneDpp LANE_DPP_CTRL[LANE_DPP_BASE] = {
    {LANE_DPP_QUAD_A, 15, 15, false}, {LANE_DPP_QUAD_B, 15, 15, false},
    {0x101, 15, 15, false}, {0x108, 15, 15, false}, {0x10f, 15, 15, false},  // row_shl 1, 8, 15
    {0x111, 15, 15, false}, {0x118, 15, 15, false}, {0x11f, 15, 15, false},  // row_shr
    {0x121, 15, 15, false}, {0x128, 15, 15, false}, {0x12f, 15, 15, false},  // row_ror
    {0x140, 15, 15, false}, {0x141, 15, 15, false},                          // row_mirror, row_half_mirror
    {0x142, 0xa, 15, false}, {0x143, 0xc, 15, false},                        // row_bcast:15, row_bcast:31
    {0x130, 15, 15, false}, {0x134, 15, 15, false}, {0x138, 15, 15, false}, {0x13c, 15, 15, false}};
constexpr int LANE_DPP_N = 2 * LANE_DPP_BASE + 2;  // 40: each keeping old, each zero-filling, two partial masks

// entry i of the control table: [0, 19) keep old, [19, 38) bound_ctrl, 38 a partial row mask, 39 a partial bank mask
AK_HOST_DEVICE constexpr LaneDpp lane_dpp(int i) {
  if (i < LANE_DPP_BASE) return LANE_DPP_CTRL[i];
  if (i < 2 * LANE_DPP_BASE) {
    LaneDpp d = LANE_DPP_CTRL[i - LANE_DPP_BASE];
    d.bound_ctrl = true;
    return d;
  }
  if (i == 2 * LANE_DPP_BASE) return LaneDpp{0x111, 0x5, 15, true};  // row_shr:1 on rows 0 and 2
  return LaneDpp{0x140, 15, 0x6, false};                              // row_mirror into banks 1 and 2
}

// where lane `l` (0..63) of the destination gets its value from
AK_HOST_DEVICE constexpr int lane_dpp_src(LaneDpp d, int l) {
  const int row = l >> 4, r = l & 15;
  if (!((d.row_mask >> row) & 1) || !((d.bank_mask >> (r >> 2)) & 1)) return LANE_SRC_OLD;
  const int invalid = d.bound_ctrl ? LANE_SRC_ZERO : LANE_SRC_OLD;
  const int c = d.ctrl, n = c & 15;
  if (c < 0x100) return (l & ~3) | ((c >> (2 * (l & 3))) & 3);
  if (c < 0x110) return r + n < 16 ? l + n : invalid;                    // row_shl: from the lane n above
  if (c < 0x120) return r >= n ? l - n : invalid;                        // row_shr: from the lane n below
  if (c < 0x130) return (l & ~15) | ((r - n) & 15);                      // row_ror
  if (c == 0x130) return l < 63 ? l + 1 : invalid;                       // wave_shl:1
  if (c == 0x134) return (l + 1) & 63;                                   // wave_rol:1
  if (c == 0x138) return l > 0 ? l - 1 : invalid;                        // wave_shr:1
  if (c == 0x13c) return (l - 1) & 63;                                   // wave_ror:1
  if (c == 0x140) return l ^ 15;
  if (c == 0x141) return l ^ 7;
  if (c == 0x142) return row > 0 ? 16 * row - 1 : invalid;               // row_bcast:15: lane 15 of the row below
  return row > 1 ? 31 : invalid;                                         // row_bcast:31
}

// v_permlane16_swap_b32 / v_permlane32_swap_b32 on the registers (A, B) = (vdst, src0). Result register
// `reg` (0: A, 1: B) of lane l is register .reg of lane .lane before the instruction.
struct LaneSwapSrc {
  int reg, lane;
};
// 16: the odd rows of A change places with the even rows of B; 32: the upper half of A with the lower half of B
AK_HOST_DEVICE constexpr LaneSwapSrc lane_swap_src(int width, int reg, int l) {
  const bool upper = (l / width) & 1;
  if (reg == 0) return upper ? LaneSwapSrc{1, l - width} : LaneSwapSrc{0, l};
  return upper ? LaneSwapSrc{1, l} : LaneSwapSrc{0, l + width};
}

// the ops of the dpp unit, in table order: the 40 controls, the two results of each swap, v_readlane
constexpr int LANE_OP_SWAP16 = LANE_DPP_N, LANE_OP_SWAP32 = LANE_DPP_N + 2, LANE_OP_READLANE = LANE_DPP_N + 4;
constexpr int LANE_DPP_OPS = LANE_DPP_N + 5;  // 45

AK_HOST_DEVICE constexpr int lane_readlane_index(uint32_t key, int wave) { return static_cast<int>(((key >> 8) + 5u * wave) & 63u); }

// ---------------------------------------------------------------------------- perm
// ds_bpermute_b32: lane t of the workgroup pulls from lane mix32(key + t) & 63 of its wave (duplicates are the rule).
AK_HOST_DEVICE inline int lane_bpermute_src(uint32_t key, int t) { return static_cast<int>(mix32(key + static_cast<uint32_t>(t)) & 63u); }

// ds_permute_b32: lane l of wave w pushes to (a l + b) mod 64, a odd: a bijection, so no push collides
AK_HOST_DEVICE constexpr int lane_permute_a(uint32_t key, int wave) { return static_cast<int>(((key >> 3) + 2u * wave) & 63u) | 1; }
AK_HOST_DEVICE constexpr int lane_permute_b(uint32_t key, int wave) { return static_cast<int>(((key >> 11) + 7u * wave) & 63u); }
AK_HOST_DEVICE constexpr int lane_permute_dst(int a, int b, int l) { return (a * l + b) & 63; }
// the lane that pushes to d: a^-1 (d - b) mod 64. a a = 1 mod 8 for odd a, and one step of Newton's
// iteration doubles the three correct bits to six.
AK_HOST_DEVICE constexpr int lane_permute_src(int a, int b, int d) {
  const int inv = (a * (2 - a * a)) & 63;
  return (inv * (d - b)) & 63;
}

// ds_swizzle_b32 offsets: bit 15 set: quad-perm mode, the permutation in bits [7:0]; else bit-mask mode on the
// lane's low five bits, and_mask [4:0], or_mask [9:5], xor_mask [14:10]: src = ((l & and) | or) ^ xor in
// each half of the wave.
constexpr int lane_swizzle_bits(int and_mask, int or_mask, int xor_mask) { return and_mask | or_mask << 5 | xor_mask << 10; }
constexpr int LANE_SWIZZLE_N = 11;
constexpr int LANE_SWIZZLE[LANE_SWIZZLE_N] = {
    0x8000 | LANE_DPP_QUAD_A, 0x8000 | 0x93,  // quad-perm [3,2,1,0] and [3,0,1,2]
    lane_swizzle_bits(31, 0, 1), lane_swizzle_bits(31, 0, 2), lane_swizzle_bits(31, 0, 4), lane_swizzle_bits(31, 0, 8),
    lane_swizzle_bits(31, 0, 16),             // the butterfly steps
    lane_swizzle_bits(28, 0, 0),              // lane 0 of each quad to the quad
    lane_swizzle_bits(31, 3, 0),              // lane 3 of each quad
    lane_swizzle_bits(31, 0, 31),             // the half reversed
    lane_swizzle_bits(23, 8, 5)};             // all three masks at once

AK_HOST_DEVICE constexpr int lane_swizzle_src(int offset, int l) {
  if (offset & 0x8000) return (l & ~3) | ((offset >> (2 * (l & 3))) & 3);
  const int j = (((l & 31) & (offset & 31)) | ((offset >> 5) & 31)) ^ ((offset >> 10) & 31);
  return (l & 32) | j;
}

constexpr int LANE_OP_BPERMUTE = 0, LANE_OP_PERMUTE = 1, LANE_OP_SWIZZLE = 2;
constexpr int LANE_PERM_OPS = 2 + LANE_SWIZZLE_N;  // 13

// ---------------------------------------------------------------------------- tr
// Each wave owns LANE_TR_SLICE bytes of LDS at wave * LANE_TR_SLICE. Lane l addresses the row at byte
// l * stride of the slice: 8 bytes (b16, b8, b4) or 12 bytes (b6) wide, the stride no power of two. A row
// holds 4, 8, 16 or 16 elements of 16, 8, 4 or 6 bits, element c at bits [c bits, (c + 1) bits) of the row
// (little-endian); element e = row * per_row + c of the tile is the low bits of mix32(key + e).
enum : int { LANE_TR_B16 = 0, LANE_TR_B8 = 1, LANE_TR_B4 = 2, LANE_TR_B6 = 3, LANE_TR_FORMS = 4 };
constexpr int LANE_TR_SLICE = 3072;
constexpr int LANE_TR_BITS[LANE_TR_FORMS] = {16, 8, 4, 6};
constexpr int LANE_TR_PER_LANE[LANE_TR_FORMS] = {4, 8, 16, 16};   // elements to a row, and to a lane's result
constexpr int LANE_TR_STRIDE[LANE_TR_FORMS] = {24, 24, 24, 48};   // bytes between the rows of two lanes
constexpr int LANE_TR_REGS[LANE_TR_FORMS] = {2, 2, 2, 3};         // result registers
constexpr int LANE_TR_REG_TOTAL = 9;

// The element that lands at position j of lane l (0..63) of the wave, as observed on an MI355X: within each
// block of 16 lanes the rows form a matrix M[16][per_row], read row-major across the block: with k = 16 / per_row,
// lane l' = l mod 16 gets M[k j + l' div per_row][l' mod per_row], j = 0 .. per_row - 1 (k = 4, 2, 1, 1 for b16,
// b8, b4, b6). So lanes 0..3 of a b16 block hold the four columns of rows 0, 4, 8, 12. (The ISA text read the
// other way, M[per_row (l' mod k) + j][l' div k]; the part does not do that.) A b6 row is 96 contiguous bits.
AK_HOST_DEVICE constexpr int lane_tr_element(int form, int l, int j) {
  const int per = LANE_TR_PER_LANE[form], k = 16 / per, lb = l & 15;
  const int row = (l & ~15) + k * j + lb / per, col = lb % per;
  return row * per + col;
}

// ---------------------------------------------------------------------------- dma
// The sweep of the direct loads over the workgroup's LDS. Wave w owns the region of LANE_DMA_REGION words at
// w * LANE_DMA_REGION and in round r uses the width of mode (w + r) mod 3: dword, dwordx3 or dwordx4.
// As observed on an MI355X, lane l of an instruction writes at base + immediate + 4 l bytes (dword) or
// base + immediate + 16 l bytes (dwordx3 and dwordx4 alike): the dwordx3 form moves 12 bytes a lane into
// 16-byte slots and leaves the fourth word of every slot alone (the expectation was a 12-byte stride). So a
// dword instruction covers 64 words and the two others 256, and in a dwordx3 region the words w with w mod 4 = 3
// are written by no instruction: they must still hold what the clear before the sweep put there. The
// immediate offset applies to the global address as well. Chunk LANE_DMA_IMM_CHUNK of every region is
// issued with the immediate offset LANE_DMA_IMM and both of its base addresses lowered by as much. LDS word
// w of workgroup b is source word b * LANE_WORDS + w, src[i] = mix32(skey + i).
constexpr int LANE_DMA_REGION = LANE_WORDS / LANE_WAVES;  // 2560 words
constexpr int LANE_DMA_IMM = 128, LANE_DMA_IMM_CHUNK = 1;
constexpr uint32_t LANE_DMA_CLEAR = 0xdeadbeefu;  // xor the round: over the whole LDS before every sweep, and no hash
constexpr int LANE_DMA_BYTES_3_ROUNDS = LANE_WAVES * (2 * 4 + 3) * LANE_DMA_REGION;  // landed in LDS by one workgroup

struct LaneDmaChunk {
  int word, width, imm;  // first word within the region, bytes a lane, immediate offset in bytes
};

AK_HOST_DEVICE constexpr int lane_dma_mode(int wave, int round) { return (wave + round % 3) % 3; }

// instructions to a region: 2560 words in chunks of 64 (dword) or 256 (dwordx3, dwordx4)
AK_HOST_DEVICE constexpr int lane_dma_chunks(int mode) { return mode == 0 ? 40 : 10; }

AK_HOST_DEVICE constexpr LaneDmaChunk lane_dma_chunk(int mode, int i) {
  return LaneDmaChunk{(mode == 0 ? 64 : 256) * i, mode == 0 ? 4 : mode == 1 ? 12 : 16, i == LANE_DMA_IMM_CHUNK ? LANE_DMA_IMM : 0};
}

// the LDS byte, relative to the chunk's first word, at which lane l's data lands
AK_HOST_DEVICE constexpr int lane_dma_lane_offset(int width, int l) { return (width == 4 ? 4 : 16) * l; }

// whether the sweep of a region in `mode` writes word w of it
AK_HOST_DEVICE constexpr bool lane_dma_written(int mode, int w) { return mode != 1 || (w & 3) != 3; }

AK_HOST_DEVICE inline uint32_t lane_dma_source_key(uint32_t seed) { return mix32(seed ^ 0x646d6121u); }

// ---------------------------------------------------------------------------- keys
// key(unit, round) = mix32(seed, block, tag + round) with the tag prefixes below
constexpr uint32_t LANE_TAG_DPP = 0x44000000u, LANE_TAG_PERM = 0x50000000u, LANE_TAG_TR = 0x58000000u;
constexpr uint32_t LANE_OLD_XOR = 0x5bd1e995u;  // old = mix32((key ^ LANE_OLD_XOR) + t)
constexpr uint32_t LANE_ROUND_MASK = 0x00ffffffu;

AK_HOST_DEVICE inline uint32_t lane_key(uint32_t seed, uint32_t block, uint32_t tag, int round) {
  return mix32(seed, block, tag + (static_cast<uint32_t>(round) & LANE_ROUND_MASK));
}

}  // namespace amdkube
