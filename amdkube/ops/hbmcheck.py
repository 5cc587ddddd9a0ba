"""Host-side reference of the HBM check (kernels/hbm_check.h, kernels/hbm_plan.h), pure numpy: the
background pattern and the seed of a chunk, one element of the march on an array of words, the plan of a
region, the self-test's slots and bits, and a model of the order in which the downward walk visits its
slots. Written from the formulas documented in the headers, never by calling the device, so the GPU tests
can hold the kernels against it."""
from __future__ import annotations

import math

import numpy as np

SLOT_BYTES = 16
PAGE_BYTES = 2 << 20
PAGE_SLOTS = PAGE_BYTES // SLOT_BYTES       # 131,072 slots of 16 bytes
CHUNK_MAX_SLOTS = 1 << 32
CHUNK_MIB_DEFAULT = 1024
FREE_FRACTION_MAX = 0.95
PLAN_RESERVE_BYTES = 16 << 20
RECORDS = 64                                # records kept, and the most self-test flips
BAD_PAGES = 32
FLIP_TAG = 0x464C4950
BLOCK = 256                                 # lanes of a workgroup of hbm_march_kernel
UNROLL = 8                                  # HBM_UNROLL: loads in flight per lane in the main loop
COUNTERS = ("errors", "bit_errors", "transient", "persistent")
_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------- the pattern
def mix32(x):
    """mix32 of kernels/gpu_common.h on a Python integer or an array of them (uint64 holding 32 bits)."""
    if isinstance(x, (int, np.integer)):
        x = int(x) & _M32
        x ^= x >> 16
        x = (x * 0x7FEB352D) & _M32
        x ^= x >> 15
        x = (x * 0x846CA68B) & _M32
        return x ^ (x >> 16)
    x = np.asarray(x, dtype=np.uint64) & np.uint64(_M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(_M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(_M32)
    return x ^ (x >> np.uint64(16))


def mix32_3(seed: int, block: int, index: int) -> int:
    """The three-argument mix32 of gpu_common.h."""
    return mix32(mix32((int(seed) ^ (0x9E3779B9 * (int(block) + 1))) & _M32) + int(index))


def chunk_seed(seed: int, round: int, chunk: int) -> int:
    """hbm_chunk_seed: the seed of chunk `chunk`'s background in round `round`."""
    return mix32_3(seed, round, chunk)


def pattern(n16: int, seed: int):
    """P: pattern() of gpu_common.h for slots 0..n16-1, as 4 * n16 uint32 words."""
    i = np.arange(n16, dtype=np.uint64)
    base = ((i * np.uint64(4)) & np.uint64(_M32)) ^ np.uint64(int(seed) & _M32) ^ ((i >> np.uint64(30)) & np.uint64(_M32))
    return np.stack([mix32(base + np.uint64(j)) for j in range(4)], axis=1).ravel().astype(np.uint32)


# ---------------------------------------------------------------------------- one element of the march
def page_of(slot: int, chunk: int = 0, chunk_bytes: int = CHUNK_MIB_DEFAULT << 20) -> int:
    """The 2 MiB page of the region that slot `slot` of chunk `chunk` lies in."""
    return (int(chunk) * int(chunk_bytes) + int(slot) * SLOT_BYTES) // PAGE_BYTES


def march_pass(words, seed: int, invert: bool, down: bool, write: bool) -> dict:
    """One launch of hbm_march_kernel over `words` (uint32, four to a slot): every word is compared with
    E = P ^ (all ones if `invert`), then, if `write`, the slot is overwritten with ~E: the complement of
    what was expected, not of what was read. A memory that returns what it holds gives `again == got`,
    so every error is persistent. `down` changes the order of the visits and nothing a healthy memory
    can show. Returns `words` after the pass, the four counters, `page_errors` (one count per 2 MiB page)
    and `records`, the set of (slot, word, got, want, again)."""
    del down
    w = np.ascontiguousarray(words, dtype=np.uint32).ravel()
    if w.size == 0 or w.size % 4:
        raise ValueError("need a whole, positive number of 16-byte words")
    n16 = w.size // 4
    want = pattern(n16, seed) ^ np.uint32(_M32 if invert else 0)
    bad = np.flatnonzero(w != want)
    diff = (w[bad] ^ want[bad]).astype(np.uint64)
    page_errors = np.bincount(bad // 4 // PAGE_SLOTS, minlength=-(-n16 // PAGE_SLOTS)).astype(np.uint32)
    return {
        "words": (~want).astype(np.uint32) if write else w.copy(),
        "errors": int(bad.size),
        "bit_errors": int(sum(bin(int(d)).count("1") for d in diff)),
        "transient": 0,
        "persistent": int(bad.size),
        "page_errors": page_errors,
        "records": {(int(k) // 4, int(k) % 4, int(w[k]), int(want[k]), int(w[k])) for k in bad},
    }


# ---------------------------------------------------------------------------- the plan
def plan(free_bytes: int, mib: int = 0, free_fraction: float = 0.0, chunk_mib: int = CHUNK_MIB_DEFAULT) -> dict:
    """hbm_plan of kernels/hbm_plan.h: {"bytes", "chunk_bytes", "chunks"}; 0 means "not given" for `mib`
    and `free_fraction`, and exactly one of them must be. ValueError for what the header refuses."""
    has_mib, has_fraction = mib != 0, free_fraction != 0
    if has_mib == has_fraction:
        raise ValueError("give the region as mib or as free_fraction, and not both")
    if has_mib and not 2 <= mib <= 1 << 30:
        raise ValueError("mib must be at least 2 (one 2 MiB page)")
    if has_fraction and not 0 < free_fraction <= FREE_FRACTION_MAX:
        raise ValueError("free fraction must be in (0, 0.95]")
    if chunk_mib < 2 or chunk_mib % 2 or chunk_mib > CHUNK_MAX_SLOTS * SLOT_BYTES >> 20:
        raise ValueError("chunk mib must be even, in [2, 65536]")
    want = int(mib) << 20 if has_mib else int(np.longdouble(free_bytes) * np.longdouble(free_fraction))
    size = want // PAGE_BYTES * PAGE_BYTES
    if size < PAGE_BYTES:
        raise ValueError("the region is smaller than one 2 MiB page")
    if free_bytes < PLAN_RESERVE_BYTES or size > free_bytes - PLAN_RESERVE_BYTES:
        raise ValueError(f"a region of {size >> 20} MiB does not fit the {free_bytes >> 20} MiB free")
    chunk_bytes = int(chunk_mib) << 20
    return {"bytes": size, "chunk_bytes": chunk_bytes,
            "chunks": [min(chunk_bytes, size - at) for at in range(0, size, chunk_bytes)]}


# ---------------------------------------------------------------------------- the self-test
def flip_slots(seed: int, n: int, n16: int) -> list[int]:
    """flip_positions(seed, n, n16) of kernels/check_core.h: the slots of chunk 0 the self-test corrupts.
    The stride is coprime to n16, so they are distinct while n <= n16."""
    seed = int(seed) & _M32
    base = seed * 2654435761 + 0x5BD1E995                          # below 2^64: no wrap to model
    stride = (((seed ^ 0x9E3779B9) * 0x85EBCA6B) % n16) | 1
    while math.gcd(stride, n16) != 1:
        stride += 2
    return [(base + i * stride) % n16 for i in range(n)]


def flip_bit(seed: int, flip: int) -> tuple[int, int]:
    """(word of the slot, bit of the word) that flip number `flip` XORs: the hash of hbm_flip_kernel."""
    h = mix32_3(seed, FLIP_TAG, flip)
    return h & 3, (h >> 2) & 31


# ---------------------------------------------------------------------------- the order of the visits
def chunk_of(n, grid, block):
    """chunk_of of gpu_common.h: [lo, hi) of workgroup `block`; an empty share has hi <= lo."""
    per = (n + grid - 1) // grid
    lo = block * per
    return lo, min(lo + per, n)


def march_visits(n16: int, grid: int, down: bool) -> list[tuple]:
    """Every load of hbm_march_kernel launched on `grid` workgroups: (slot, workgroup, lane, "main" or
    "tail", iteration of that loop), in the form of tests/stream_ref.py. Lane t walks the distances
    t, t + 256, ... from the end of its workgroup's share it starts at: the low end going up, the top slot
    going down."""
    out = []
    for blk in range(grid):
        lo, hi = chunk_of(n16, grid, blk)
        if lo >= hi:
            continue
        length = hi - lo
        at = (lambda d: hi - 1 - d) if down else (lambda d: lo + d)
        for t in range(BLOCK):
            d, it = t, 0
            while d + (UNROLL - 1) * BLOCK < length:
                out += [(at(d + u * BLOCK), blk, t, "main", it) for u in range(UNROLL)]
                d += UNROLL * BLOCK
                it += 1
            it = 0
            while d < length:
                out.append((at(d), blk, t, "tail", it))
                d += BLOCK
                it += 1
    return out
