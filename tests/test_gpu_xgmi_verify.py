"""GPU tier: the verifier of xgmi-probe's all-reduce (kernels/xgmi_verify.h) through the probe binary and
through the in-process ops, against the numpy mirror (amdkube/ops/xgmiverify.py) and for 1 to 64 ranks on
one GPU: the all-reduce result is built on the host from what the fill kernel wrote for each rank.

The tests that start child processes come first, as in test_gpu.py; each child is a fresh process. torch
and the HIP ops are imported inside the tests, as in test_gpu_mfma_check.py.

No tolerance anywhere: every value and partial sum is a multiple of 0.5 below 2^23 (xgmi_pattern.h), so
every comparison is bitwise or an exact count. The one inequality is the 99 % floor of the displacement
test; the expected miss rate is 1 in 4096, and tests/test_xgmi_verify_ref.py holds the seeds and shapes
used here to that floor on the CPU.
"""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from amdkube.ops import xgmiverify as xv
from tests.test_xgmi_verify_ref import DISPLACEMENT_FLOOR, RANKS, SEEDS, SHAPES, SWAP, bits, swap_blocks

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
PROBE_ELEMENTS = 262144                   # --max-mib 1
shape_id = lambda s: f"{s[0]}x{s[1]}"     # noqa: E731


def _probe(*args):
    return subprocess.run([os.path.join(BIN, "xgmi-probe"), *args], capture_output=True, text=True, timeout=120)


def _json(r):
    try:    # RCCL may write its banner to stdout before the one JSON line
        return json.loads(r.stdout[r.stdout.index("{\"gpus\""):r.stdout.rindex("}") + 1])
    except ValueError as e:
        raise AssertionError(f"xgmi-probe output is not JSON ({e}): {r.stdout[:800]!r} {r.stderr[-800:]!r}")


# ---------------------------------------------------------------- the binary
def test_probe_clean_run_reports_the_whole_verify_block():
    r = _probe("--max-mib", "1", "--iters", "1", "--no-p2p")
    assert r.returncode == 0, (r.stdout, r.stderr)
    x = _json(r)
    v = x["verify"]
    assert v["wrong"] == 0 and v["elements"] == PROBE_ELEMENTS and v["ranks"] == x["gpus"] >= 1, x
    assert v["first_errors"] == [] and v["seed"] == 0x5EED and v["selftest_flips"] == 0, x
    assert len(x["devices"]) == x["gpus"] and len(x["allreduce"]) == 1 and len(x["p2p_gbps"]) == x["gpus"], x


@pytest.mark.parametrize("seed_arg,seed", [("0x5eed", 0x5EED), ("12345", 12345)])
@pytest.mark.parametrize("flips", [1, 16, 37])
def test_probe_reports_exactly_the_selftest_flips(flips, seed_arg, seed):
    r = _probe("--max-mib", "1", "--iters", "1", "--no-p2p", "--seed", seed_arg, "--selftest-flips", str(flips))
    assert r.returncode == 5, (r.returncode, r.stdout, r.stderr)
    assert f"xgmi-probe: all-reduce returned {flips} wrong elements" in r.stderr, r.stderr
    x = _json(r)
    v, gpus = x["verify"], x["gpus"]
    assert v["wrong"] == flips == v["selftest_flips"] and v["seed"] == seed and v["elements"] == PROBE_ELEMENTS, x
    pos = xv.flip_positions(seed, flips, PROBE_ELEMENTS)
    predicted = {(i % gpus, pos[i]) for i in range(flips)}
    recs = v["first_errors"]
    pairs = {(e["rank"], e["index"]) for e in recs}
    assert len(recs) == min(flips, xv.RECORDS) == len(pairs) and pairs <= predicted, (recs, sorted(predicted))
    for e in recs:
        assert e["got"] ^ e["want"] == 1 and e["want"] == int(bits(xv.want(seed, gpus, e["index"]))), e


BAD_ARGS = [
    ["--bogus"], ["-h"], ["1"], ["--no-p2p", "1"], ["--max-mib=1"],                              # unknown
    ["--max-mib"], ["--iters"], ["--seed"], ["--selftest-flips"], ["--no-p2p", "--iters"],       # no value
    ["--max-mib", "0"], ["--max-mib", "65537"], ["--max-mib", "-1"], ["--max-mib", "1x"], ["--max-mib", "0x10"],
    ["--max-mib", " 1"], ["--max-mib", "+1"], ["--max-mib", ""], ["--max-mib", "1.0"], ["--max-mib", "99999999999999999999"],
    ["--iters", "0"], ["--iters", "10001"], ["--iters", "abc"], ["--iters", "--no-p2p"], ["--iters", "2e1"],
    ["--seed", "0x"], ["--seed", "0xg"], ["--seed", "5eed"], ["--seed", "4294967296"], ["--seed", "0x100000000"], ["--seed", "-1"],
    ["--selftest-flips", "65"], ["--selftest-flips", "-1"], ["--selftest-flips", "0x1"], ["--selftest-flips", "many"],
]


def test_probe_refuses_bad_arguments_before_it_touches_the_gpu():
    for args in BAD_ARGS:
        r = _probe("--max-mib", "1", *args)
        assert r.returncode == 2 and r.stdout == "", (args, r.returncode, r.stdout, r.stderr)
        assert r.stderr.startswith("xgmi-probe: bad argument") and r.stderr.count("\n") == 1, (args, r.stderr)


# ---------------------------------------------------------------- fill
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fill_is_the_mirrors_value_bit_for_bit(shape):
    from amdkube.ops import hip
    count, grid = shape
    e = np.arange(count, dtype=np.uint64)
    for seed in SEEDS:
        for rank in (0, 1, 63):
            got = hip.xgmi_fill(count, rank, seed, grid=grid)
            assert got.dtype == np.float32 and got.shape == (count,)
            assert np.array_equal(bits(got), bits(xv.value(seed, rank, e))), (seed, rank)


# ---------------------------------------------------------------- the reference all-reduce
@functools.lru_cache(maxsize=None)
def device_sums(seed, count, grid):
    """{n: the float32 sum of hip.xgmi_fill over ranks 0 .. n-1} for n in RANKS, read-only: the result of
    an all-reduce over n ranks, built once. The float64 sum of the same arrays agrees exactly at every n,
    so the reference is exact by itself, whatever the kernels under test say."""
    from amdkube.ops import hip
    s32, s64, out = np.zeros(count, np.float32), np.zeros(count, np.float64), {}
    for rank in range(max(RANKS)):
        v = hip.xgmi_fill(count, rank, seed, grid=grid)
        s32 += v
        s64 += v.astype(np.float64)
        if rank + 1 in RANKS:
            assert np.array_equal(s32.astype(np.float64), s64), (seed, count, rank + 1)
            out[rank + 1] = s32.copy()
            out[rank + 1].setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_count_passes_the_sum_of_n_ranks_for_n_up_to_64(shape):
    from amdkube.ops import hip
    count, grid = shape
    e = np.arange(count, dtype=np.uint64)
    for seed in SEEDS:
        for n, s in device_sums(seed, count, grid).items():
            assert np.array_equal(bits(s), bits(xv.want(seed, n, e))), (seed, n)
            r = hip.xgmi_count_wrong(s, n, seed, grid=grid)
            assert r == {"wrong": 0, "records": []}, (seed, n, r)


# ---------------------------------------------------------------- count on a wrong sum
BIG = SHAPES[-1]                           # three whole trips of the production grid and a tail trip of 5 elements
TAIL = 3 * 262144                          # the first element of that tail trip
NAN, INF = 0x7FC00000, 0x7F800000


def _corruptions():
    rng = np.random.default_rng(20251)
    many = rng.choice(BIG[0], size=1000, replace=False)
    return {
        "one_ulp": {1000: None},
        "nan_inf_zero": {31: NAN, 70001: INF, 500000: 0},
        "tail_trip": {TAIL + 2: None},
        "first_and_last": {0: None, BIG[0] - 1: None},
        "thousand_random": {int(i): None for i in many},
        "all_of_them": {1000: None, 31: NAN, 70001: INF, 500000: 0, TAIL + 2: None, 0: None, BIG[0] - 1: None,
                        **{int(i): None for i in many}},
    }


@pytest.mark.parametrize("name", ["one_ulp", "nan_inf_zero", "tail_trip", "first_and_last", "thousand_random", "all_of_them"])
@pytest.mark.parametrize("n", [1, 8])
def test_count_counts_each_wrong_element_once_and_records_where(n, name):
    """A value of None is the element's own bits with the low mantissa bit flipped: one ulp."""
    from amdkube.ops import hip
    seed, (count, grid) = SEEDS[0], BIG
    where = _corruptions()[name]
    words = bits(device_sums(seed, count, grid)[n]).copy()
    for i, b in where.items():
        words[i] = words[i] ^ np.uint32(1) if b is None else np.uint32(b)
    r = hip.xgmi_count_wrong(words.view(np.float32), n, seed, grid=grid)
    assert r["wrong"] == len(where), (r["wrong"], len(where))
    recs = r["records"]
    assert len(recs) == min(len(where), xv.RECORDS) == len({e["index"] for e in recs})
    for e in recs:
        assert e["index"] in where and e["got"] == int(words[e["index"]]), e
        assert e["want"] == int(bits(xv.want(seed, n, e["index"]))), e
    # and through a tail of one workgroup's loop at a few KiB: 1541 = 3 * 512 + 5 on two workgroups
    count, grid = SHAPES[4]
    words = bits(device_sums(seed, count, grid)[n]).copy()
    words[[0, 1536, 1540]] ^= np.uint32(1)
    r = hip.xgmi_count_wrong(words.view(np.float32), n, seed, grid=grid)
    assert r["wrong"] == 3 and {e["index"] for e in r["records"]} == {0, 1536, 1540}, r


@pytest.mark.parametrize("n", [1, 7])
def test_count_with_one_rank_too_many_sees_every_element_wrong(n):
    from amdkube.ops import hip
    seed = SEEDS[1]
    for count, grid in (SHAPES[4], SHAPES[5]):
        r = hip.xgmi_count_wrong(device_sums(seed, count, grid)[n], n + 1, seed, grid=grid)
        assert r["wrong"] == count and len(r["records"]) == min(count, xv.RECORDS), r["wrong"]
        for e in r["records"]:
            assert e["want"] == int(bits(xv.want(seed, n + 1, e["index"]))) != e["got"]
            assert e["got"] == int(bits(xv.want(seed, n, e["index"])))


# ---------------------------------------------------------------- displacement
@pytest.mark.parametrize("seed", SEEDS)
def test_count_sees_a_displaced_block_of_the_sum(seed):
    """A stale chunk, a chunk in another chunk's slot: the distances are multiples of 7, which the pattern
    this one replaced, (rank + 1) + 0.5 * (e % 7), could not see."""
    from amdkube.ops import hip
    count, grid = BIG
    n = 4
    s = device_sums(seed, count, grid)[n]
    w = xv.want(seed, n, np.arange(count, dtype=np.uint64))
    first, second, length = SWAP
    for what, moved_sum, moved in (("roll 7", np.roll(s, 7), count), ("roll 14", np.roll(s, 14), count),
                                   ("swap", swap_blocks(s, first, second, length), 2 * length)):
        r = hip.xgmi_count_wrong(moved_sum, n, seed, grid=grid)
        print(f"seed {seed:#x} {what}: {r['wrong']} of {moved} moved elements wrong")
        assert DISPLACEMENT_FLOOR * moved <= r["wrong"] <= moved, (what, r["wrong"], moved)
        assert r["wrong"] == int(np.count_nonzero(moved_sum != w)), what


# ---------------------------------------------------------------- refusals
def test_ops_refuse_ranks_and_grids_out_of_range():
    from amdkube._native import _hipops
    from amdkube.ops import hip
    one = np.ones(4, np.float32)
    for call in (lambda m: m.xgmi_count_wrong(one, 0, 0x5EED, 0, 0), lambda m: m.xgmi_count_wrong(one, 65, 0x5EED, 0, 0),
                 lambda m: m.xgmi_fill(4, -1, 0x5EED, 0, 0), lambda m: m.xgmi_fill(4, 64, 0x5EED, 0, 0),
                 lambda m: m.xgmi_fill(4, 0, 0x5EED, 0, 65537), lambda m: m.xgmi_count_wrong(one, 1, 0x5EED, 0, 65537),
                 lambda m: m.xgmi_fill(4, 0, 0x5EED, 0, -1)):
        for module in (hip, _hipops):      # the wrapper's check, and the runner's own behind it
            with pytest.raises(ValueError):
                call(module)
    assert hip.xgmi_count_wrong(hip.xgmi_fill(4, 63, grid=65536), 1, grid=65536)["wrong"] == 4
