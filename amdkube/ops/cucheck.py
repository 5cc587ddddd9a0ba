"""Host-side reference of the per-CU check (kernels/cu_check.h), pure numpy: the LDS march pattern,
the vector-ALU operands and their exact results, the inputs of the transcendental unit and the
decoding of a workgroup's location. Written from the formulas documented in the header, never by
calling the device, so the GPU tests can hold the kernel against it."""
from __future__ import annotations

import numpy as np

LDS_BYTES = 163840
LDS_WORDS = LDS_BYTES // 4          # 40,960 words, 10,240 16-byte slots
THREADS = 1024                      # lanes of one workgroup
CHAIN = 16
TRANS_FUNCS = ("exp2", "log2", "rcp", "rsq", "sqrt")
TRANS_SETS = 4
UNITS = ("lds", "valu", "trans")
MAX_FLIPS = 4096
_M32 = np.uint64(0xFFFFFFFF)


def units_mask(units) -> int:
    """("lds", "trans") → 5; ValueError on an unknown, repeated or missing name."""
    if isinstance(units, str):
        units = tuple(units.split(","))
    units = tuple(units)
    bad = [u for u in units if u not in UNITS]
    if bad or not units or len(set(units)) != len(units):
        raise ValueError(f"unknown unit {bad[0]!r}: expected some of {', '.join(UNITS)}" if bad else
                         f"units must name each of {', '.join(UNITS)} at most once and one at least, got {units!r}")
    return sum(1 << UNITS.index(u) for u in units)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def key(seed: int, block: int, tag):
    """mix32(seed, block, tag) of kernels/gpu_common.h, as uint64 holding 32-bit values."""
    s = mix32((int(seed) ^ (0x9E3779B9 * (int(block) + 1))) & 0xFFFFFFFF)
    return mix32((s + np.asarray(tag, dtype=np.uint64)) & _M32)


def lds_pattern(seed: int, block: int, round: int, pass_: int = 1):
    """The 40,960 words of the LDS image as pass `pass_` (1, 2 or 3) of round `round` writes it:
    P, ~P, P with P(wa) = wa * mul + add mod 2^32."""
    if pass_ not in (1, 2, 3):
        raise ValueError("only passes 1, 2 and 3 write the image")
    k = int(key(seed, block, 0x4C000000 + int(round)))
    mul, add = np.uint64(k | 1), mix32(k ^ 0x85EBCA6B)
    p = (np.arange(LDS_WORDS, dtype=np.uint64) * mul + add) & _M32
    if pass_ == 2:
        p ^= _M32
    return p.astype(np.uint32)


def valu_operands(seed: int, block: int):
    """uint32 [1024, 12]: a0 b0 c0 a1 b1 c1 (a < 2^12, b < 2^11, c < 2^23), wa wb wc (< 2^26), and the
    chain's x, m, k, for every lane of the workgroup."""
    t = np.arange(THREADS, dtype=np.uint64)
    h = [key(seed, block, np.uint64(0x56000000) + np.uint64(8) * t + np.uint64(n)) for n in range(8)]
    u = np.uint64
    cols = [h[0] & u(0xFFF), (h[0] >> u(12)) & u(0x7FF), h[1] & u(0x7FFFFF),
            h[2] & u(0xFFF), (h[2] >> u(12)) & u(0x7FF), h[3] & u(0x7FFFFF),
            h[4] & u(0x3FFFFFF), h[5] & u(0x3FFFFFF), h[6] & u(0x3FFFFFF), h[7], h[4] | u(1), h[5]]
    return np.stack(cols, axis=1).astype(np.uint32)


def valu_expected(ops):
    """From valu_operands: int64 [1024, 4] with a0 b0 + c0, a1 b1 + c1, wa wb + wc and the result of the
    wrapping chain (16 times x = x m + k mod 2^32), all exact."""
    o = np.asarray(ops).astype(np.int64)
    x, m, k = (np.asarray(ops)[:, i].astype(np.uint64) for i in (9, 10, 11))
    for _ in range(CHAIN):
        x = (x * m + k) & _M32
    return np.stack([o[:, 0] * o[:, 1] + o[:, 2], o[:, 3] * o[:, 4] + o[:, 5], o[:, 6] * o[:, 7] + o[:, 8],
                     x.astype(np.int64)], axis=1)


def trans_inputs(seed: int, block: int):
    """float32 [1024, 5, 4]: per lane, the inputs of exp2, log2, rcp, rsq and sqrt (TRANS_FUNCS), four
    each. Waves w and w ^ 1 share their inputs."""
    t = np.arange(THREADS, dtype=np.uint64)
    g = np.uint64(64) * (t >> np.uint64(7)) + (t & np.uint64(63))
    out = np.empty((THREADS, len(TRANS_FUNCS), TRANS_SETS), np.float32)
    for f in range(len(TRANS_FUNCS)):
        for s in range(TRANS_SETS):
            h = key(seed, block, np.uint64(0x54000000) + np.uint64(32) * g + np.uint64(4 * f + s))
            if f == 0:
                v = ((h * np.uint64(10485760)) >> np.uint64(32)).astype(np.int64) - 5242880
                out[:, f, s] = (v.astype(np.float64) * 2.0 ** -18).astype(np.float32)       # exact
                continue
            top = h >> np.uint64(23)
            if f == 1:
                i = (top * np.uint64(38)) >> np.uint64(9)
                e = np.where(i < 19, np.uint64(107) + i, np.uint64(109) + i)
            else:
                e = np.uint64(107) + ((top * np.uint64(40)) >> np.uint64(9))
            out[:, f, s] = ((e << np.uint64(23)) | (h & np.uint64(0x7FFFFF))).astype(np.uint32).view(np.float32)
    return out


def trans_reference(x):
    """float64 values of the five functions on trans_inputs' array."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([np.exp2(x[:, 0]), np.log2(x[:, 1]), 1.0 / x[:, 2], 1.0 / np.sqrt(x[:, 3]), np.sqrt(x[:, 4])], axis=1)


def decode_location(hw_id: int, xcc_id: int) -> dict:
    """(xcc, se, sh, cu) from the raw HW_ID and XCC_ID words: XCC_ID [3:0]; HW_ID CU_ID [11:8],
    SH_ID [12], SE_ID [15:13]. The wave, SIMD, pipe, queue and VM fields are not part of a location."""
    hw_id, xcc_id = int(hw_id), int(xcc_id)
    return {"xcc": xcc_id & 15, "se": (hw_id >> 13) & 7, "sh": (hw_id >> 12) & 1, "cu": (hw_id >> 8) & 15}
