"""Host-side reference of the atomic-unit check (kernels/atomic_check.h, kernels/atomic_plan.h), pure numpy:
the slot map, the operands of every op and the tables one scatter round leaves behind, reduced with
np.add.at, np.minimum.at and the like in int64, uint64 and float64. Written from the formulas documented
in the header, never by calling the device, so the GPU tests can hold the kernels against it."""
from __future__ import annotations

import numpy as np

from .cucheck import mix32

WG = 256                            # lanes of a workgroup
STEPS = 4                           # T of the device
MAX_BLOCKS = 1024
MAX_FLIPS = 64
DEFAULT_BLOCKS = 512
DEFAULT_CONTENTION = (1, 64, 4096)
CAS_MAX_CONTENTION = 64
UNITS = ("int", "fp", "ret", "lds")
OPS = {"int": ("add_u32", "add_u64", "and", "or", "xor", "smin", "smax", "umin", "umax", "umin_u64", "umax_u64"),
       "fp": ("add_f32", "add_f64", "min_f64", "max_f64", "pk_add_bf16", "pk_add_f16"),
       "ret": ("ticket", "cas_add")}
LDS_OPS = OPS["int"] + OPS["fp"] + ("cas_add",)
VIEWS = {"add_f32": np.float32, "add_f64": np.float64, "min_f64": np.float64, "max_f64": np.float64,
         "smin": np.int32, "smax": np.int32}                # how the dumped bits of an op are to be read
_M32 = np.uint64(0xFFFFFFFF)
_U = np.uint64


def units_mask(units) -> int:
    """("int", "lds") → 9; ValueError on an unknown, repeated or missing name."""
    if isinstance(units, str):
        units = tuple(units.split(","))
    units = tuple(units)
    bad = [u for u in units if u not in UNITS]
    if bad or not units or len(set(units)) != len(units):
        raise ValueError(f"unknown unit {bad[0]!r}: expected some of {', '.join(UNITS)}" if bad else
                         f"units must name each of {', '.join(UNITS)} at most once and one at least, got {units!r}")
    return sum(1 << UNITS.index(u) for u in units)


def check_contention(contention, blocks: int) -> list[int]:
    levels = [int(c) for c in contention]
    for c in levels:
        if c < 1 or c & (c - 1) or c > blocks * WG:
            raise ValueError(f"contention {c} is not a power of two in [1, {blocks * WG}]")
    if not levels:
        raise ValueError("the contention list is empty")
    return levels


def global_ops(units, contention: int) -> list[str]:
    """The ops with a global table at this contention: the CAS-loop add runs at c <= 64 only."""
    return [op for u in UNITS[:3] if u in units for op in OPS[u] if op != "cas_add" or contention <= CAS_MAX_CONTENTION]


def checked_count(blocks: int, contention, rounds: int, units=UNITS) -> int:
    """Slot-ops a run checks: per round and level S slots of every global op, and SL slots of every LDS op
    in every workgroup."""
    total = 0
    for c in contention:
        total += (blocks * WG // c) * len(global_ops(units, c))
        if "lds" in units:
            total += blocks * (WG // min(c, WG)) * len(LDS_OPS)
    return total * rounds


def _mix3(seed, block, index):
    """mix32(seed, block, index) of kernels/check_core.h, elementwise."""
    s = mix32((np.asarray(seed, dtype=_U) ^ (_U(0x9E3779B9) * (np.asarray(block, dtype=_U) + _U(1)))) & _M32)
    return mix32((s + np.asarray(index, dtype=_U)) & _M32)


def slot_map(seed: int, round: int, step: int):
    """(mul, add) of a step: p = (g mul + add) & (G - 1)."""
    k = int(_mix3(seed, round, 0x41000000 + step))
    return k | 1, int(mix32(k ^ 0x85EBCA6B))


def positions(seed: int, round: int, step: int, G: int):
    """p of every lane g in 0..G-1."""
    mul, add = slot_map(seed, round, step)
    return ((np.arange(G, dtype=_U) * _U(mul) + _U(add)) & _M32) & _U(G - 1)


def values(seed: int, round: int, step: int, g):
    key = int(_mix3(seed, round, 0x4B000000))
    return _mix3(key, g, step)


def f32_mask(n: int) -> int:
    lim = (1 << 24) // n
    return (1 << (lim.bit_length() - 1)) - 1


def operands(v, j, n: int) -> dict:
    """What a contribution of value v (uint64 holding 32 bits) and rank j adds to every op."""
    w = (v * _U(0x85EBCA6B)) & _M32
    a64 = v * _U(0x9E3779B97F4A7C15)                                  # wraps mod 2^64
    s32 = lambda x: x.astype(np.uint32).view(np.int32).astype(np.int64)  # noqa: E731
    gate8, gate16 = j < 8, j < 16
    return {
        "add_u32": v, "add_u64": a64, "and": ~(_U(1) << (v & _U(31))) & _M32, "or": _U(1) << ((v >> _U(5)) & _U(31)),
        "xor": w, "smin": s32(v), "smax": s32(w), "umin": w, "umax": v, "umin_u64": a64, "umax_u64": (w << _U(32)) | v,
        "add_f32": ((v >> _U(7)) & _U(f32_mask(n))).astype(np.float64), "add_f64": w.astype(np.float64),
        "min_f64": s32(w).astype(np.float64), "max_f64": s32(v).astype(np.float64),
        "bf_lo": np.where(gate8, 1 + (v & _U(7)), 0).astype(np.int64),
        "bf_hi": np.where(gate8, 1 + ((v >> _U(3)) & _U(7)), 0).astype(np.int64),
        "h_lo": np.where(gate16, 1 + ((v >> _U(8)) & _U(31)), 0).astype(np.int64),
        "h_hi": np.where(gate16, 1 + ((v >> _U(13)) & _U(31)), 0).astype(np.int64),
        "cas_add": v ^ _U(0x5BD1E995),
    }


def _reduce(slots: int, contributions, n: int) -> dict:
    """The tables of `slots` slots after every (slot, operands) pair of `contributions` arrived, as the
    device dumps them: uint32 or uint64 words, the ops of VIEWS in their own type, the packed ops as bits."""
    t = {"add_u32": np.zeros(slots, np.uint64), "add_u64": np.zeros(slots, np.uint64),
         "and": np.full(slots, 0xFFFFFFFF, np.uint64), "or": np.zeros(slots, np.uint64), "xor": np.zeros(slots, np.uint64),
         "smin": np.full(slots, 2**31 - 1, np.int64), "smax": np.full(slots, -2**31, np.int64),
         "umin": np.full(slots, 0xFFFFFFFF, np.uint64), "umax": np.zeros(slots, np.uint64),
         "umin_u64": np.full(slots, 2**64 - 1, np.uint64), "umax_u64": np.zeros(slots, np.uint64),
         "add_f32": np.zeros(slots, np.float64), "add_f64": np.zeros(slots, np.float64),
         "min_f64": np.full(slots, np.inf), "max_f64": np.full(slots, -np.inf),
         "bf_lo": np.zeros(slots, np.int64), "bf_hi": np.zeros(slots, np.int64),
         "h_lo": np.zeros(slots, np.int64), "h_hi": np.zeros(slots, np.int64), "cas_add": np.zeros(slots, np.uint64)}
    how = {"and": np.bitwise_and, "or": np.bitwise_or, "xor": np.bitwise_xor, "smin": np.minimum, "smax": np.maximum,
           "umin": np.minimum, "umax": np.maximum, "umin_u64": np.minimum, "umax_u64": np.maximum, "min_f64": np.minimum,
           "max_f64": np.maximum}
    for slot, o in contributions:
        for name, table in t.items():
            how.get(name, np.add).at(table, slot, o[name])
    assert t["add_f32"].max() < 2**24 and t["add_f64"].max() < 2**53 and max(t["bf_lo"].max(), t["bf_hi"].max()) <= 256 \
        and max(t["h_lo"].max(), t["h_hi"].max()) <= 2048, "the operand bounds of the header do not hold"
    u32 = lambda x: (x.astype(np.uint64) & _M32).astype(np.uint32)  # noqa: E731
    bf = lambda x: x.astype(np.float32).view(np.uint32) >> 16       # noqa: E731  (integers up to 256: exact)
    f16 = lambda x: x.astype(np.float16).view(np.uint16).astype(np.uint32)  # noqa: E731  (up to 2048: exact)
    out = {k: u32(t[k]) for k in ("add_u32", "and", "or", "xor", "umin", "umax", "cas_add")}
    out.update({k: t[k] for k in ("add_u64", "umin_u64", "umax_u64")})
    out.update({k: t[k].astype(np.int32).view(np.uint32) for k in ("smin", "smax")})
    out["add_f32"] = t["add_f32"].astype(np.float32).view(np.uint32)
    out.update({k: t[k].view(np.uint64) for k in ("add_f64", "min_f64", "max_f64")})
    out["pk_add_bf16"] = bf(t["bf_lo"]) | bf(t["bf_hi"]) << 16
    out["pk_add_f16"] = f16(t["h_lo"]) | f16(t["h_hi"]) << 16
    out["ticket"] = np.full(slots, n, np.uint32)
    return {k: v.view(VIEWS.get(k, v.dtype)) for k, v in out.items()}


def global_tables(G: int, contention: int, seed: int = 0x5EED, round: int = 0, units=UNITS, steps: int = STEPS) -> dict:
    """Every global table after one scatter round of G lanes, by op name, and `order`: per slot the sorted
    ids i G + g of its n contributions, shape (S, n)."""
    S, n = G // contention, contention * steps
    lg = S.bit_length() - 1
    g = np.arange(G, dtype=_U)
    contributions, ids = [], []
    for i in range(steps):
        p = positions(seed, round, i, G)
        slot = (p & _U(S - 1)).astype(np.int64)
        contributions.append((slot, operands(values(seed, round, i, g), p >> _U(lg), n)))
        ids.append((slot, i * G + np.arange(G, dtype=np.int64)))
    t = _reduce(S, contributions, n)
    out = {op: t[op] for op in global_ops(units, contention)}
    if "ret" in units:
        slot, who = np.concatenate([s for s, _ in ids]), np.concatenate([w for _, w in ids])
        by_slot = np.lexsort((who, slot))
        out["order"] = who[by_slot].reshape(S, n).astype(np.uint32)
    return out


def lds_tables(block: int, contention: int, seed: int = 0x5EED, round: int = 0, steps: int = STEPS) -> dict:
    """The LDS tables of workgroup `block` after its lanes' contributions, by op name."""
    cl = min(contention, WG)
    SL, n = WG // cl, cl * steps
    lg = SL.bit_length() - 1
    g = _U(block * WG) + np.arange(WG, dtype=_U)
    contributions = []
    for i in range(steps):
        p = positions(seed, round, i, WG)          # the low 8 bits of the global p: the map of lane t = g & 255
        contributions.append(((p & _U(SL - 1)).astype(np.int64), operands(values(seed, round, i, g), p >> _U(lg), n)))
    t = _reduce(SL, contributions, n)
    return {op: t[op] for op in LDS_OPS}
