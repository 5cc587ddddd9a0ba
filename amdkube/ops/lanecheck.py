"""Host-side reference of the lane check (kernels/lane_check.h, kernels/lane_plan.h), pure numpy: for
(seed, block) the result tables of the `dpp` and `perm` units, the registers of the four transposing LDS
reads and the LDS image after the `dma` sweep of round 0. Written from the formulas documented in the two
headers, never by calling the device, so the GPU tests can hold the kernel against it."""
from __future__ import annotations

import numpy as np

from .cucheck import key, mix32

THREADS = 1024
WAVES = 16
LDS_WORDS = 40960
UNITS = ("dpp", "perm", "tr", "dma")
MAX_FLIPS = 4096
SRC_ZERO, SRC_OLD = -1, -2
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64

TAG_DPP, TAG_PERM, TAG_TR = 0x44000000, 0x50000000, 0x58000000
OLD_XOR = 0x5BD1E995

# (ctrl, row_mask, bank_mask): every control once, then all again with bound_ctrl, then two partial masks
_DPP_BASE = [(0x1B, 15, 15), (0x4E, 15, 15), (0x101, 15, 15), (0x108, 15, 15), (0x10F, 15, 15), (0x111, 15, 15),
             (0x118, 15, 15), (0x11F, 15, 15), (0x121, 15, 15), (0x128, 15, 15), (0x12F, 15, 15), (0x140, 15, 15),
             (0x141, 15, 15), (0x142, 0xA, 15), (0x143, 0xC, 15), (0x130, 15, 15), (0x134, 15, 15), (0x138, 15, 15),
             (0x13C, 15, 15)]
DPP_TABLE = ([(*c, False) for c in _DPP_BASE] + [(*c, True) for c in _DPP_BASE]
             + [(0x111, 0x5, 15, True), (0x140, 15, 0x6, False)])
DPP_OPS = len(DPP_TABLE) + 5          # + both registers of the two swaps, v_readlane
OP_SWAP16, OP_SWAP32, OP_READLANE = len(DPP_TABLE), len(DPP_TABLE) + 2, len(DPP_TABLE) + 4


def _bits(a, o, x):
    return a | o << 5 | x << 10


SWIZZLE = [0x8000 | 0x1B, 0x8000 | 0x93, _bits(31, 0, 1), _bits(31, 0, 2), _bits(31, 0, 4), _bits(31, 0, 8),
           _bits(31, 0, 16), _bits(28, 0, 0), _bits(31, 3, 0), _bits(31, 0, 31), _bits(23, 8, 5)]
PERM_OPS = 2 + len(SWIZZLE)

TR_FORMS = ("b16", "b8", "b4", "b6")
TR_BITS = (16, 8, 4, 6)
TR_PER_LANE = (4, 8, 16, 16)
TR_REGS = (2, 2, 2, 3)
TR_FIRST_REG = (0, 2, 4, 6)

DMA_REGION = LDS_WORDS // WAVES
DMA_CLEAR = 0xDEADBEEF


def units_mask(units) -> int:
    """"dpp,tr" or ("dpp", "tr") → 5; ValueError on an unknown, repeated or missing name."""
    if isinstance(units, str):
        units = tuple(units.split(","))
    units = tuple(units)
    bad = [u for u in units if u not in UNITS]
    if bad or not units or len(set(units)) != len(units):
        raise ValueError(f"unknown unit {bad[0]!r}: expected some of {', '.join(UNITS)}" if bad else
                         f"units must name each of {', '.join(UNITS)} at most once and one at least, got {units!r}")
    return sum(1 << UNITS.index(u) for u in units)


def dpp_src(entry, lanes=None):
    """The source lane of every destination lane 0..63 under a DPP_TABLE entry: >= 0, SRC_ZERO or SRC_OLD."""
    ctrl, row_mask, bank_mask, bound = entry
    l = np.arange(64) if lanes is None else np.asarray(lanes)
    row, r, n = l >> 4, l & 15, ctrl & 15
    invalid = SRC_ZERO if bound else SRC_OLD
    if ctrl < 0x100:
        src = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3)
    elif ctrl < 0x110:
        src = np.where(r + n < 16, l + n, invalid)
    elif ctrl < 0x120:
        src = np.where(r >= n, l - n, invalid)
    elif ctrl < 0x130:
        src = (l & ~15) | ((r - n) & 15)
    elif ctrl == 0x130:
        src = np.where(l < 63, l + 1, invalid)
    elif ctrl == 0x134:
        src = (l + 1) & 63
    elif ctrl == 0x138:
        src = np.where(l > 0, l - 1, invalid)
    elif ctrl == 0x13C:
        src = (l - 1) & 63
    elif ctrl == 0x140:
        src = l ^ 15
    elif ctrl == 0x141:
        src = l ^ 7
    elif ctrl == 0x142:
        src = np.where(row > 0, 16 * row - 1, invalid)
    else:
        src = np.where(row > 1, 31, invalid)
    enabled = ((row_mask >> row) & 1).astype(bool) & ((bank_mask >> (r >> 2)) & 1).astype(bool)
    return np.where(enabled, src, SRC_OLD)


def swap_src(width: int, reg: int):
    """(register, lane) that result register `reg` of v_permlane{width}_swap takes, for the lanes 0..63."""
    l = np.arange(64)
    upper = ((l // width) & 1).astype(bool)
    if reg == 0:
        return np.where(upper, 1, 0), np.where(upper, l - width, l)
    return np.where(upper, 1, 0), np.where(upper, l, l + width)


def swizzle_src(offset: int):
    l = np.arange(64)
    if offset & 0x8000:
        return (l & ~3) | ((offset >> (2 * (l & 3))) & 3)
    return (l & 32) | ((((l & 31) & (offset & 31)) | ((offset >> 5) & 31)) ^ ((offset >> 10) & 31))


def _values(k: int, t):
    return mix32((_U(k) + np.asarray(t, dtype=np.uint64)) & _M32)


def dpp_table(seed: int, block: int, round: int = 0):
    """uint32 [1024, 45]: what every lane of the workgroup holds after each op of the dpp unit."""
    k = int(key(seed, block, TAG_DPP + round))
    ko = k ^ OLD_XOR
    t = np.arange(THREADS)
    wb, l = t & ~63, t & 63
    v, old = _values(k, t), _values(ko, t)
    out = np.empty((THREADS, DPP_OPS), np.uint64)
    for i, entry in enumerate(DPP_TABLE):
        s = dpp_src(entry)[l]
        out[:, i] = np.where(s >= 0, v[wb + np.maximum(s, 0)], np.where(s == SRC_ZERO, _U(0), old))
    for op, width in ((OP_SWAP16, 16), (OP_SWAP32, 32)):
        for reg in (0, 1):
            which, lane = swap_src(width, reg)
            out[:, op + reg] = np.where(which[l] == 1, old[wb + lane[l]], v[wb + lane[l]])
    idx = ((k >> 8) + 5 * (t >> 6)) & 63
    out[:, OP_READLANE] = v[wb + idx]
    return out.astype(np.uint32)


def perm_table(seed: int, block: int, round: int = 0):
    """uint32 [1024, 13]: ds_bpermute, ds_permute, then the swizzles."""
    k = int(key(seed, block, TAG_PERM + round))
    t = np.arange(THREADS)
    wb, l, wave = t & ~63, t & 63, t >> 6
    v = _values(k, t)
    out = np.empty((THREADS, PERM_OPS), np.uint64)
    out[:, 0] = v[wb + (_values(k ^ OLD_XOR, t) & _U(63)).astype(np.int64)]
    a = (((k >> 3) + 2 * wave) & 63) | 1
    b = ((k >> 11) + 7 * wave) & 63
    inv = (a * (2 - a * a)) & 63
    out[:, 1] = v[wb + ((inv * (l - b)) & 63)]
    for i, offset in enumerate(SWIZZLE):
        out[:, 2 + i] = v[wb + swizzle_src(offset)[l]]
    return out.astype(np.uint32)


def tr_element(form: int, l, j):
    """The element of the wave's tile at position j of lane l: lane_tr_element of lane_plan.h."""
    per = TR_PER_LANE[form]
    k, lb = 16 // per, l & 15
    return ((l & ~15) + k * j + lb // per) * per + lb % per


def tr_registers(seed: int, block: int, round: int = 0):
    """uint32 [1024, 9]: the registers of ds_read_b64_tr_b16, _b8, _b4 (two each) and ds_read_b96_tr_b6 (three)."""
    t = np.arange(THREADS)
    wave, l = t >> 6, t & 63
    out = np.zeros((THREADS, 9), np.uint64)
    for f in range(4):
        k = int(key(seed, block, TAG_TR + (f << 24) + round))
        per, bits = TR_PER_LANE[f], TR_BITS[f]
        wide = [0] * THREADS                                   # Python integers: up to 96 bits
        for j in range(per):
            x = _values(k, wave * 64 * per + tr_element(f, l, j)) & _U((1 << bits) - 1)
            wide = [w | int(e) << (j * bits) for w, e in zip(wide, x)]
        for r in range(TR_REGS[f]):
            out[:, TR_FIRST_REG[f] + r] = [(w >> (32 * r)) & 0xFFFFFFFF for w in wide]
    return out.astype(np.uint32)


def dma_mode(wave, round: int):
    """0 dword, 1 dwordx3, 2 dwordx4: the width wave `wave` sweeps its region with in round `round`."""
    return (np.asarray(wave) + round % 3) % 3


def dma_image(seed: int, block: int, round: int = 0):
    """uint32 [40960]: the LDS after the sweep: word w holds src[40960 block + w], but for the fourth word of
    every 16-byte slot in a dwordx3 region, which no direct load writes and the clear value stays in."""
    w = np.arange(LDS_WORDS)
    skey = int(mix32(int(seed) ^ 0x646D6121))
    img = _values(skey, block * LDS_WORDS + w)
    hole = (dma_mode(w // DMA_REGION, round) == 1) & (w % 4 == 3)
    return np.where(hole, _U(DMA_CLEAR ^ round), img).astype(np.uint32)


def flip_positions(seed: int, count: int, blocks: int, units=UNITS):
    """The self-test's (unit, block, element) of flips 0..count-1, as check_core.h places them: flip i goes to
    the i mod n-th enabled unit at (base + i stride) mod (blocks * elems), elems = 1024 lanes or 40960 words."""
    import math
    names = [u for u in UNITS if u in units]
    small, large = blocks * THREADS, blocks * LDS_WORDS
    base = (seed * 2654435761 + 0x5BD1E995) & 0xFFFFFFFFFFFFFFFF
    stride = ((((seed ^ 0x9E3779B9) & 0xFFFFFFFF) * 0x85EBCA6B) % small) | 1
    while math.gcd(stride, large) != 1:
        stride += 2
    out = []
    for i in range(count):
        u = names[i % len(names)]
        elems = LDS_WORDS if u == "dma" else THREADS
        p = (base + i * stride) % (blocks * elems)
        out.append((u, p // elems, p % elems))
    return out


def decode_location(hw_id: int, xcc_id: int) -> dict:
    """(xcc, se, sh, cu, simd) from the raw words of a wave: cucheck.decode_location and SIMD_ID, HW_ID [5:4]."""
    from .cucheck import decode_location as cu
    return {**cu(hw_id, xcc_id), "simd": (int(hw_id) >> 4) & 3}
