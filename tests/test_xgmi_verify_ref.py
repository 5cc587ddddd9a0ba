"""The arithmetic of xgmi-probe's all-reduce verifier on the CPU: the self-test of kernels/xgmi_pattern.h
(plain and under ASan/UBSan), its printed table against the numpy mirror (amdkube/ops/xgmiverify.py), and
what the pattern is for: a block of the sum that lands in another place is seen, at the seeds and shapes
tests/test_gpu_xgmi_verify.py uses. Every comparison is bitwise or an exact count; the one inequality is the
99 % floor of the displacement tests (the expected miss rate is 1 in 4096)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from amdkube.ops import hbmcheck
from amdkube.ops import xgmiverify as xv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))

SEEDS = (0x5EED, 12345)
# (count, grid) of the GPU tests: zero, one, a partial and several trips of the grid-stride loop (256 lanes
# a workgroup, 1024 workgroups at grid 0)
SHAPES = ((1, 0), (255, 1), (256, 1), (257, 1), (1541, 2), (262144 + 3, 0), (3 * 262144 + 5, 0))
RANKS = (1, 2, 3, 4, 7, 8, 64)
DISPLACEMENT_FLOOR = 0.99


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def host_sum(seed, n, count):
    """The all-reduce result built from the mirror's values: the float32 sum over ranks 0 .. n-1."""
    e = np.arange(count, dtype=np.uint64)
    s = np.zeros(count, np.float32)
    for rank in range(n):
        s += xv.value(seed, rank, e)
    return s


def swap_blocks(a, first, second, length):
    out = a.copy()
    out[first:first + length], out[second:second + length] = a[second:second + length], a[first:first + length]
    return out


# where the two swapped 4096-element blocks start: both multiples of 7, as is their distance
SWAP = (7 * 100, 7 * 40000, 4096)


@pytest.fixture(scope="module")
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


@pytest.mark.parametrize("binary", ["xgmi-pattern-selftest", "xgmi-pattern-selftest-asan"])
def test_the_selftest_runs_clean_and_its_table_is_the_mirrors(built, binary):
    r = subprocess.run([os.path.join(BIN, binary)], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("OK"), r.stdout[-2000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    rows = [ln.split() for ln in lines[:-1]]
    assert len(rows) == 4 * 9 * (3 + 5) and {row[0] for row in rows} == {"value", "want"}
    for kind, seed, k, e, got in rows:
        mirror = (xv.value if kind == "value" else xv.want)(int(seed), int(k), int(e))
        assert int(bits(mirror)) == int(got), (kind, seed, k, e)
    assert any(int(row[3]) >= 1 << 32 for row in rows)


def test_mix32_is_the_projects_and_the_term_is_made_of_it():
    assert xv.mix32(1) == 0x688990C0 and xv.mix32(0) == 0
    assert xv.mix32 is hbmcheck.mix32
    for seed in SEEDS + (0, 0xFFFFFFFF):
        for e in (0, 1, 4095, 262143, (1 << 32) - 1, 1 << 32, (7 << 32) + 3, (1 << 64) - 1):
            assert int(xv.term(seed, e)) == hbmcheck.mix32_3(seed, e >> 32, e & 0xFFFFFFFF) & 4095
    e = np.arange(1 << 16, dtype=np.uint64)
    t = xv.term(SEEDS[0], e)
    assert t.dtype == np.uint32 and int(t.max()) < xv.TERMS and len(np.unique(t)) == xv.TERMS
    assert not np.array_equal(t, xv.term(SEEDS[0], e + np.uint64(1 << 32)))      # the high half counts
    assert not np.array_equal(t, xv.term(SEEDS[1], e))


def test_values_sum_to_want_in_float32_and_float64_for_every_rank_count():
    count = 5000
    e = np.arange(count, dtype=np.uint64)
    for seed in SEEDS:
        s32, s64 = np.zeros(count, np.float32), np.zeros(count, np.float64)
        for n in range(1, xv.MAX_RANKS + 1):
            v = xv.value(seed, n - 1, e)
            assert v.dtype == np.float32
            s32 += v
            s64 += v.astype(np.float64)
            w = xv.want(seed, n, e)
            assert w.dtype == np.float32 and np.array_equal(bits(s32), bits(w)) and np.array_equal(s32.astype(np.float64), s64)
        assert float(s32.max()) <= 2080 + 0.5 * 64 * 4095 < 2 ** 23


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("distance", [7, 14, 4096, 1])
def test_a_displaced_sum_differs_from_want_almost_everywhere(seed, distance):
    count = SHAPES[-1][0]
    e = np.arange(count, dtype=np.uint64)
    for n in (1, 4):
        s, w = host_sum(seed, n, count), xv.want(seed, n, e)
        assert np.array_equal(bits(s), bits(w))
        wrong = int(np.count_nonzero(np.roll(s, distance) != w))
        assert DISPLACEMENT_FLOOR * count <= wrong <= count, (wrong, count)
        first, second, length = SWAP
        wrong = int(np.count_nonzero(swap_blocks(s, first, second, length) != w))
        assert DISPLACEMENT_FLOOR * 2 * length <= wrong <= 2 * length, wrong


def test_the_pattern_this_one_replaced_saw_none_of_that():
    """(rank + 1) + 0.5 * (e % 7): a block a multiple of 7 elements from its place is what was expected there.
    Of a rolled sum only the few elements that wrapped round the end differ."""
    count, n = SHAPES[-1][0], 4
    e = np.arange(count)
    old_want = np.float32(0.5 * n * (n + 1)) + np.float32(0.5 * n) * (e % 7).astype(np.float32)
    assert count % 7
    for distance in (7, 14):
        assert int(np.count_nonzero(np.roll(old_want, distance) != old_want)) <= distance
    assert np.array_equal(swap_blocks(old_want, *SWAP), old_want)


def test_flip_positions_and_refusals():
    for seed in SEEDS:
        for flips in (0, 1, 16, 37, 64):
            pos = xv.flip_positions(seed, flips, 262144)
            assert len(pos) == flips == len(set(pos)) and all(0 <= p < 262144 for p in pos)
        assert xv.flip_positions(seed, 37, 262144) == hbmcheck.flip_slots(seed, 37, 262144)
    xv.check_args(ranks=1, rank=0, grid=0)
    xv.check_args(ranks=64, rank=63, grid=65536)
    for bad in ({"ranks": 0}, {"ranks": 65}, {"rank": -1}, {"rank": 64}, {"grid": 65537}, {"grid": -1}):
        with pytest.raises(ValueError):
            xv.check_args(**bad)
