// CPU self-test of kernels/lane_plan.h against naive loops: every source-lane map stays in range, the declared
// bijections are bijections, each transpose map is a permutation of the elements its block of 16 lanes
// addresses, and the dma plan writes every LDS word exactly once per sweep but for the fourth word of the
// dwordx3 slots, which it must not write. Built plain and under ASan/UBSan (native/build.py --sanitize).
#include <cstdio>
#include <set>
#include <vector>

#include "../kernels/lane_plan.h"

using namespace amdkube;

static int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      std::printf("FAIL %s: ", #cond);       \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
    }                                        \
  } while (0)

static bool bijection(const std::vector<int>& m) {
  std::set<int> seen(m.begin(), m.end());
  return seen.size() == m.size() && *seen.begin() == 0 && *seen.rbegin() == static_cast<int>(m.size()) - 1;
}

// the DPP source of lane l spelled out control by control, with no shared arithmetic
static int naive_dpp(LaneDpp d, int l) {
  const int row = l / 16, r = l % 16;
  if (!(d.row_mask & (1 << row)) || !(d.bank_mask & (1 << (r / 4)))) return LANE_SRC_OLD;
  const int inv = d.bound_ctrl ? LANE_SRC_ZERO : LANE_SRC_OLD;
  switch (d.ctrl) {
    case 0x1b: { const int q[4] = {3, 2, 1, 0}; return l - l % 4 + q[l % 4]; }
    case 0x4e: { const int q[4] = {2, 3, 0, 1}; return l - l % 4 + q[l % 4]; }
    case 0x101: case 0x108: case 0x10f: { const int n = d.ctrl - 0x100; return r + n <= 15 ? l + n : inv; }
    case 0x111: case 0x118: case 0x11f: { const int n = d.ctrl - 0x110; return r - n >= 0 ? l - n : inv; }
    case 0x121: case 0x128: case 0x12f: { const int n = d.ctrl - 0x120; return 16 * row + (r + 16 - n) % 16; }
    case 0x130: return l == 63 ? inv : l + 1;
    case 0x134: return (l + 1) % 64;
    case 0x138: return l == 0 ? inv : l - 1;
    case 0x13c: return (l + 63) % 64;
    case 0x140: return 16 * row + 15 - r;
    case 0x141: return 16 * row + 8 * (r / 8) + 7 - r % 8;
    case 0x142: return row == 0 ? inv : 16 * row - 1;
    case 0x143: return row < 2 ? inv : 31;
  }
  return -99;
}

int main() {
  // dpp: range, agreement with the naive table, every control taken both ways, a partial mask of each kind
  int bound = 0, keep = 0, part_row = 0, part_bank = 0;
  for (int i = 0; i < LANE_DPP_N; ++i) {
    const LaneDpp d = lane_dpp(i);
    (d.bound_ctrl ? bound : keep)++;
    part_row += d.row_mask != 15 && d.ctrl != 0x142 && d.ctrl != 0x143;
    part_bank += d.bank_mask != 15;
    for (int l = 0; l < 64; ++l) {
      const int s = lane_dpp_src(d, l);
      CHECK(s >= LANE_SRC_OLD && s < 64, "dpp %d lane %d src %d", i, l, s);
      CHECK(s == naive_dpp(d, l), "dpp %d (ctrl 0x%x) lane %d: %d, naive %d", i, d.ctrl, l, s, naive_dpp(d, l));
      if (s == LANE_SRC_ZERO) CHECK(d.bound_ctrl, "dpp %d zero-fills without bound_ctrl", i);
    }
  }
  CHECK(bound == LANE_DPP_BASE + 1 && keep == LANE_DPP_BASE + 1 && part_row == 1 && part_bank == 1, "table shape %d %d %d %d", bound,
        keep, part_row, part_bank);
  // the swaps: the two result registers together hold every (register, lane) once
  for (int width : {16, 32}) {
    std::set<int> seen;
    for (int reg = 0; reg < 2; ++reg)
      for (int l = 0; l < 64; ++l) {
        const LaneSwapSrc s = lane_swap_src(width, reg, l);
        CHECK(s.reg >= 0 && s.reg < 2 && s.lane >= 0 && s.lane < 64, "swap%d reg %d lane %d", width, reg, l);
        seen.insert(64 * s.reg + s.lane);
        const int naive_reg = (l / width) % 2, naive_lane = reg == naive_reg ? l : reg == 0 ? l - width : l + width;
        CHECK(s.reg == naive_reg && s.lane == naive_lane, "swap%d reg %d lane %d: (%d, %d)", width, reg, l, s.reg, s.lane);
      }
    CHECK(seen.size() == 128, "swap%d is no bijection", width);
  }
  // readlane, bpermute, permute over many keys and every wave
  for (uint32_t k = 0; k < 4096; ++k) {
    const uint32_t key = mix32(k);
    for (int w = 0; w < LANE_WAVES; ++w) {
      const int idx = lane_readlane_index(key, w);
      CHECK(idx >= 0 && idx < 64, "readlane index %d", idx);
      const int a = lane_permute_a(key, w), b = lane_permute_b(key, w);
      CHECK((a & 1) && a < 64 && b >= 0 && b < 64, "permute a %d b %d", a, b);
      std::vector<int> dst(64);
      for (int l = 0; l < 64; ++l) {
        dst[l] = lane_permute_dst(a, b, l);
        CHECK(dst[l] == (a * l + b) % 64, "permute dst");
        const int s = lane_bpermute_src(key, 64 * w + l);
        CHECK(s >= 0 && s < 64, "bpermute src %d", s);
      }
      CHECK(bijection(dst), "permute a %d b %d is no bijection", a, b);
      for (int l = 0; l < 64; ++l) CHECK(lane_permute_src(a, b, dst[l]) == l, "permute inverse a %d b %d lane %d", a, b, l);
    }
  }
  {  // the pull map has duplicates: that is the case it is there for
    std::set<int> pulled;
    for (int l = 0; l < 64; ++l) pulled.insert(lane_bpermute_src(mix32(1), l));
    CHECK(pulled.size() < 64, "bpermute map without duplicates");
  }
  // swizzle: range, the butterflies, and the naive bit-mask rule
  for (int i = 0; i < LANE_SWIZZLE_N; ++i)
    for (int l = 0; l < 64; ++l) {
      const int off = LANE_SWIZZLE[i], s = lane_swizzle_src(off, l);
      CHECK(s >= 0 && s < 64 && s / 32 == l / 32, "swizzle %d lane %d src %d", i, l, s);
      if (off & 0x8000) {
        CHECK(s / 4 == l / 4 && s % 4 == ((off >> (2 * (l % 4))) & 3), "swizzle quad %d lane %d", i, l);
      } else {
        const int a = off & 31, o = (off >> 5) & 31, x = (off >> 10) & 31;
        int j = 0;
        for (int bit = 0; bit < 5; ++bit) {
          int v = (l >> bit) & 1;
          if (!((a >> bit) & 1)) v = 0;
          if ((o >> bit) & 1) v = 1;
          if ((x >> bit) & 1) v ^= 1;
          j |= v << bit;
        }
        CHECK(s == 32 * (l / 32) + j, "swizzle mask %d lane %d: %d, naive %d", i, l, s, 32 * (l / 32) + j);
      }
    }
  for (int step = 0; step < 5; ++step)
    for (int l = 0; l < 64; ++l) CHECK(lane_swizzle_src(LANE_SWIZZLE[2 + step], l) == (l ^ (1 << step)), "butterfly %d", step);
  // tr: the rows fit the slice, and each block of 16 lanes reads exactly the elements of its 16 rows, once each
  for (int f = 0; f < LANE_TR_FORMS; ++f) {
    const int per = LANE_TR_PER_LANE[f];
    CHECK(per * LANE_TR_BITS[f] == 32 * LANE_TR_REGS[f], "form %d row width", f);
    CHECK(63 * LANE_TR_STRIDE[f] + 4 * LANE_TR_REGS[f] <= LANE_TR_SLICE && (LANE_TR_STRIDE[f] & (LANE_TR_STRIDE[f] - 1)) != 0 &&
              LANE_TR_STRIDE[f] % (f == LANE_TR_B6 ? 16 : 8) == 0, "form %d stride", f);
    for (int blk = 0; blk < 4; ++blk) {
      std::vector<int> got;
      for (int l = 16 * blk; l < 16 * blk + 16; ++l)
        for (int j = 0; j < per; ++j) got.push_back(lane_tr_element(f, l, j) - 16 * blk * per);
      CHECK(bijection(got), "form %d block %d is no permutation of its elements", f, blk);
    }
    // the map as observed: position j of lane l' is row k j + l' / per, column l' % per
    for (int l = 0; l < 16; ++l)
      for (int j = 0; j < per; ++j) {
        const int e = lane_tr_element(f, l, j);
        CHECK(e / per == (16 / per) * j + l / per && e % per == l % per, "form %d lane %d position %d: element %d", f, l, j, e);
      }
  }
  CHECK(LANE_WAVES * LANE_TR_SLICE <= LANE_LDS_BYTES, "tr slices");
  // dma: per round, every LDS word is written once, the dwordx3 holes never; all banks see dwordx4 within 3 rounds
  std::vector<int> x4(LANE_WORDS, 0);
  long long bytes = 0;
  for (int round = 0; round < 3; ++round) {
    std::vector<int> writes(LANE_WORDS, 0);
    for (int w = 0; w < LANE_WAVES; ++w) {
      const int mode = lane_dma_mode(w, round);
      CHECK(mode >= 0 && mode < 3, "mode");
      int with_imm = 0;
      for (int i = 0; i < lane_dma_chunks(mode); ++i) {
        const LaneDmaChunk c = lane_dma_chunk(mode, i);
        with_imm += c.imm != 0;
        CHECK(4 * (w * LANE_DMA_REGION + c.word) - c.imm >= 0, "base below the LDS");
        for (int l = 0; l < 64; ++l)
          for (int b = 0; b < c.width; b += 4) {
            const int word = w * LANE_DMA_REGION + c.word + (lane_dma_lane_offset(c.width, l) + b) / 4;
            CHECK(word >= w * LANE_DMA_REGION && word < (w + 1) * LANE_DMA_REGION, "word %d leaves region %d", word, w);
            if (word >= 0 && word < LANE_WORDS) {
              ++writes[word];
              if (c.width == 16) x4[word] = 1;
              bytes += 4;
            }
          }
      }
      CHECK(with_imm == 1, "one chunk of a region has the immediate offset");
    }
    for (int word = 0; word < LANE_WORDS; ++word) {
      const int mode = lane_dma_mode(word / LANE_DMA_REGION, round);
      const int want = lane_dma_written(mode, word % LANE_DMA_REGION) ? 1 : 0;
      CHECK(writes[word] == want, "round %d word %d written %d times, want %d", round, word, writes[word], want);
      CHECK(want == 1 || (mode == 1 && word % 4 == 3), "round %d word %d", round, word);
    }
  }
  for (int word = 0; word < LANE_WORDS; ++word) CHECK(x4[word], "word %d never written by dwordx4", word);
  CHECK(bytes == LANE_DMA_BYTES_3_ROUNDS, "bytes of three rounds %lld", bytes);
  if (failures) {
    std::printf("lane-plan-selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("lane-plan-selftest: ok\n");
  return 0;
}
