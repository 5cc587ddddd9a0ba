"""The numpy reference of the atomic-unit check (amdkube/ops/atomiccheck.py) against a naive loop over
lanes in plain Python integers, and kernels/atomic_plan.h through its stand-alone self-test built plain and
with ASan/UBSan (native/atomic_plan_selftest.cpp says what it checks). CPU tier."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from amdkube.ops import atomiccheck as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))
M32, M64 = 0xFFFFFFFF, 2**64 - 1


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


@pytest.mark.parametrize("binary", ["atomic-plan-selftest", "atomic-plan-selftest-asan"])
def test_atomic_plan_selftest(binary):
    r = subprocess.run([os.path.join(BIN, binary)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def mix(x):
    x ^= x >> 16
    x = x * 0x7FEB352D & M32
    x ^= x >> 15
    x = x * 0x846CA68B & M32
    return x ^ x >> 16


def mix3(seed, block, index):
    return mix((mix((seed ^ 0x9E3779B9 * (block + 1)) & M32) + index) & M32)


def s32(x):
    return x - 2**32 if x & 0x80000000 else x


def bits(fmt_in, fmt_out, x):
    return struct.unpack(fmt_out, struct.pack(fmt_in, x))[0]


def naive(G, c, seed, rnd, T):
    """Lane after lane, step after step, as the header's formulas say; Python integers and floats only."""
    S, n = G // c, c * T
    fm = 1
    while fm * 2 <= (1 << 24) // n:
        fm *= 2
    t = {"add_u32": [0] * S, "add_u64": [0] * S, "and": [M32] * S, "or": [0] * S, "xor": [0] * S, "smin": [2**31 - 1] * S,
         "smax": [-2**31] * S, "umin": [M32] * S, "umax": [0] * S, "umin_u64": [M64] * S, "umax_u64": [0] * S,
         "add_f32": [0] * S, "add_f64": [0] * S, "min_f64": [float("inf")] * S, "max_f64": [float("-inf")] * S,
         "bf": [(0, 0)] * S, "f16": [(0, 0)] * S, "ticket": [0] * S, "cas_add": [0] * S}
    order = [[] for _ in range(S)]
    key = mix3(seed, rnd, 0x4B000000)
    for i in range(T):
        k = mix3(seed, rnd, 0x41000000 + i)
        mul, add = k | 1, mix(k ^ 0x85EBCA6B)
        for g in range(G):
            p = (g * mul + add) & M32 & (G - 1)
            s, j = p & (S - 1), p // S
            v = mix3(key, g, i)
            w = v * 0x85EBCA6B & M32
            a64 = v * 0x9E3779B97F4A7C15 & M64
            t["add_u32"][s] = (t["add_u32"][s] + v) & M32
            t["add_u64"][s] = (t["add_u64"][s] + a64) & M64
            t["and"][s] &= ~(1 << (v & 31)) & M32
            t["or"][s] |= 1 << ((v >> 5) & 31)
            t["xor"][s] ^= w
            t["smin"][s] = min(t["smin"][s], s32(v))
            t["smax"][s] = max(t["smax"][s], s32(w))
            t["umin"][s] = min(t["umin"][s], w)
            t["umax"][s] = max(t["umax"][s], v)
            t["umin_u64"][s] = min(t["umin_u64"][s], a64)
            t["umax_u64"][s] = max(t["umax_u64"][s], w << 32 | v)
            t["add_f32"][s] += (v >> 7) & (fm - 1)
            t["add_f64"][s] += w
            t["min_f64"][s] = min(t["min_f64"][s], float(s32(w)))
            t["max_f64"][s] = max(t["max_f64"][s], float(s32(v)))
            lo, hi = t["bf"][s]
            t["bf"][s] = (lo + (1 + (v & 7) if j < 8 else 0), hi + (1 + ((v >> 3) & 7) if j < 8 else 0))
            lo, hi = t["f16"][s]
            t["f16"][s] = (lo + (1 + ((v >> 8) & 31) if j < 16 else 0), hi + (1 + ((v >> 13) & 31) if j < 16 else 0))
            t["ticket"][s] += 1
            t["cas_add"][s] = (t["cas_add"][s] + (v ^ 0x5BD1E995)) & M32
            order[s].append(i * G + g)
    assert max(t["add_f32"]) < 2**24 and max(max(x) for x in t["bf"]) <= 256 and max(max(x) for x in t["f16"]) <= 2048
    t["add_f32"] = [float(x) for x in t["add_f32"]]
    t["add_f64"] = [float(x) for x in t["add_f64"]]
    t["pk_add_bf16"] = [bits("<f", "<I", float(lo)) >> 16 | bits("<f", "<I", float(hi)) >> 16 << 16 for lo, hi in t.pop("bf")]
    t["pk_add_f16"] = [bits("<e", "<H", float(lo)) | bits("<e", "<H", float(hi)) << 16 for lo, hi in t.pop("f16")]
    return t, [sorted(o) for o in order]


@pytest.mark.parametrize("c", (1, 8, 64))
def test_the_reference_equals_a_naive_loop(c):
    G, T, seed, rnd = 64, 2, 0xC0FFEE, 3
    ref = ac.global_tables(G, c, seed, rnd, steps=T)
    want, order = naive(G, c, seed, rnd, T)
    assert set(ref) == set(want) | {"order"}
    for op, column in want.items():
        assert ref[op].tolist() == column, op
    assert ref["order"].tolist() == order


def test_the_closed_form_of_the_checked_count():
    assert ac.checked_count(4, (1, 64, 1024), 2) == 2 * ((1024 + 16) * 19 + 18 + 4 * 18 * (256 + 4 + 1))
    assert ac.checked_count(1, (256,), 1, ("int", "lds")) == 11 + 18
