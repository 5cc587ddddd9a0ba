// What xgmi-probe's ranks put into the all-reduce and what every rank must hold afterwards. Plain C++17
// with no HIP include, usable on host and device, so native/xgmi_pattern_selftest.cpp checks it on the CPU,
// plain and under ASan/UBSan; kernels/xgmi_verify.h has the kernels that fill and count with it.
//
//   term(seed, e)        = mix32(seed, e >> 32, e & 0xffffffff) & 4095: hashed from both halves of the
//                          64-bit element index, so the value says where in the buffer it belongs. A block
//                          of the result that lands anywhere but in its place agrees with what is expected
//                          there in one element of 4096 on average, whatever the distance.
//   value(seed, rank, e) = (rank + 1) + 0.5 * term          what rank `rank` contributes
//   want(seed, n, e)     = 0.5 * n * (n + 1) + 0.5 * n * term     the sum over ranks 0 .. n-1
//
// Exactness: for n <= XGMI_MAX_RANKS = 64 every value, every partial sum of values over any subset of the
// ranks and both products of `want` are multiples of 0.5 of at most 2080 + 0.5 * 64 * 4095 = 133,120,
// far below the 2^23 up to which fp32 holds every multiple of 0.5. So the fp32 sum is exact in whatever
// order and grouping a collective reduces, a fused multiply-add rounds nothing either, and the verifier
// compares with != and no tolerance.
#pragma once

#include <cstdint>

#include "check_core.h"

namespace amdkube {

constexpr int XGMI_MAX_RANKS = 64;
constexpr uint32_t XGMI_TERM_MASK = 4095;

AK_HOST_DEVICE inline uint32_t xgmi_term(uint32_t seed, uint64_t e) {
  return mix32(seed, static_cast<uint32_t>(e >> 32), static_cast<uint32_t>(e)) & XGMI_TERM_MASK;
}

AK_HOST_DEVICE inline float xgmi_value(uint32_t seed, int rank, uint64_t e) {
  return static_cast<float>(rank + 1) + 0.5f * static_cast<float>(xgmi_term(seed, e));
}

AK_HOST_DEVICE inline float xgmi_want(uint32_t seed, int n, uint64_t e) {
  return 0.5f * static_cast<float>(n) * static_cast<float>(n + 1) +
         0.5f * static_cast<float>(n) * static_cast<float>(xgmi_term(seed, e));
}

}  // namespace amdkube
