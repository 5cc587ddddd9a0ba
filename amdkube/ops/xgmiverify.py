"""Host-side reference of xgmi-probe's all-reduce verifier (kernels/xgmi_pattern.h, kernels/xgmi_verify.h),
pure numpy: the hashed term of an element, what a rank contributes, what the sum over n ranks must be, and
the elements the self-test flips. Written from the formulas documented in the header, never by calling the
device, so the GPU tests can hold the kernels against it.

Every value and every partial sum is a multiple of 0.5 of at most 2080 + 0.5 * 64 * 4095 = 133,120 for up
to 64 ranks, far below 2^23, so float32 holds all of them exactly and a sum is the same in any order."""
from __future__ import annotations

import numpy as np

from .hbmcheck import flip_slots, mix32           # the one mix32 and flip_positions of kernels/check_core.h

MAX_RANKS = 64
TERMS = 4096                                      # term(seed, e) is in [0, TERMS)
RECORDS = 16                                      # records kept per count
MAX_FLIPS = 64
GRID_MAX = 65536
SEED = 0x5EED
_M32 = np.uint64(0xFFFFFFFF)


def term(seed: int, e):
    """xgmi_term: mix32(seed, e >> 32, e & 0xffffffff) & 4095, the three-argument mix32, as uint32. `e` is
    an element index or an array of them, below 2^64."""
    e = np.asarray(e, dtype=np.uint64)
    hi, lo = e >> np.uint64(32), e & _M32
    inner = mix32(np.uint64(int(seed) & 0xFFFFFFFF) ^ ((np.uint64(0x9E3779B9) * (hi + np.uint64(1))) & _M32))
    return (mix32((inner + lo) & _M32) & np.uint64(TERMS - 1)).astype(np.uint32)


def value(seed: int, rank: int, e):
    """xgmi_value: what rank `rank` puts into element e, float32."""
    return np.float32(int(rank) + 1) + np.float32(0.5) * term(seed, e).astype(np.float32)


def want(seed: int, n: int, e):
    """xgmi_want: what every rank must hold in element e after a sum over n ranks, float32."""
    n = int(n)
    return np.float32(0.5 * n * (n + 1)) + np.float32(0.5 * n) * term(seed, e).astype(np.float32)


def flip_positions(seed: int, flips: int, count: int) -> list[int]:
    """flip_positions(seed, flips, count) of kernels/check_core.h: flip i of the probe's self-test corrupts this
    element of rank i % ranks. Distinct while flips <= count."""
    return flip_slots(seed, flips, count)


def check_args(ranks: int | None = None, rank: int | None = None, grid: int = 0) -> None:
    """What the host runners of kernels/xgmi_verify.h refuse, as ValueError."""
    if ranks is not None and not 1 <= int(ranks) <= MAX_RANKS:
        raise ValueError(f"ranks must be in [1, {MAX_RANKS}]")
    if rank is not None and not 0 <= int(rank) < MAX_RANKS:
        raise ValueError(f"rank must be in [0, {MAX_RANKS})")
    if not 0 <= int(grid) <= GRID_MAX:
        raise ValueError(f"grid must be in [0, {GRID_MAX}] (0: the production grid)")
