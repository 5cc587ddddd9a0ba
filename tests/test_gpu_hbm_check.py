"""GPU tier: the HBM check (kernels/hbm_check.h) through every layer: one launch of the march kernel on
caller data against the numpy reference (amdkube/ops/hbmcheck.py), bit for bit and field for field; the
whole check in process; its self-test, which corrupts the check's own buffer; and hbm-check as a program.

The march launches run the shapes of tests/stream_ref.py with the test's own grid, so a few KiB reach the
8-deep main loop, a wave split between main loop and tail, ragged and empty shares, in both directions.
No test allocates more than 64 MiB, but the one of `--free-fraction 0.001`, whose size the device decides.
No tolerances: every comparison is exact."""
import collections
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from amdkube.ops import hbmcheck as hc
from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
SEEDS = (0x5EED, 0xC0FFEE11)
MIB = 1 << 20
COUNTS = ("errors", "bit_errors", "transient", "persistent")
MAX_ITEMS = 56            # injected slots: one word each, one of them 3 more: at most 59 <= 64 records


@functools.lru_cache(maxsize=None)
def cus():
    from amdkube.ops import hip
    return hip.device_info(0)["cu_count"]


def launched(n16, grid):
    return sr.chunked_grid(n16, grid, cus(), sr.HBM_COPY_BLOCKS_PER_CU)


def record_set(records):
    return {(e["slot"], e["word"], e["got"], e["want"], e["again"]) for e in records}


def compare(got, want, what):
    """A march launch on the device against the reference: words, counters, per-page counts, records."""
    assert got["words"].dtype == np.uint32 and np.array_equal(got["words"], want["words"]), what
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, what
    assert got["records_dropped"] == 0 and len(got["records"]) == want["errors"], what
    assert record_set(got["records"]) == want["records"], what
    assert got["page_errors"].tolist() == want["page_errors"].tolist(), what
    assert all((e["round"], e["pass"], e["chunk"]) == (0, 0, 0) for e in got["records"]), what


def injected_items(n16, grid):
    """Where a wrong loop bound would show, going up or down: slot 0, the last slot, both sides of every
    boundary between two workgroups' shares, the last lane of the main loop and the first of the tail
    (stream_ref.edge_items), and the same places counted from the top of each share, where the downward
    walk has them. Thinned evenly to MAX_ITEMS where the grid has hundreds of shares."""
    items = set(sr.edge_items(n16, grid))
    for lo, hi in sr.chunks(n16, grid):
        items |= {lo + hi - 1 - i for i in list(items) if lo <= i < hi}
    items = sorted(items)
    if len(items) > MAX_ITEMS:
        keep = np.linspace(0, len(items) - 1, MAX_ITEMS).round().astype(int)
        items = sorted({items[k] for k in keep})       # the first and the last are among them
    return items


def injected(base, n16, grid):
    """`base` with one bit flipped in one word of every injected item, several bits in one word, and all
    four words of the last slot wrong."""
    rng = np.random.default_rng(4 * n16 + grid)
    items = injected_items(n16, grid)
    bad = base.copy()
    for i in items:
        bad[4 * i + int(rng.integers(4))] ^= np.uint32(1) << np.uint32(rng.integers(32))
    mid = items[len(items) // 2]
    bad[4 * mid + 1] = base[4 * mid + 1] ^ np.uint32(0x80F00101)
    last = items[-1]
    bad[4 * last:4 * last + 4] = base[4 * last:4 * last + 4] ^ np.array([1 << 3, 1 << 9, 0x11, 1 << 31], np.uint32)
    assert last == n16 - 1 and items[0] == 0 and int((bad != base).sum()) <= hc.RECORDS
    return bad


# ---------------------------------------------------------------------------- one launch of the march kernel
@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
def test_march_pass_is_the_reference(shape):
    from amdkube.ops import hip
    n16, grid, _ = shape
    seed = SEEDS[(n16 + grid) % 2]
    for invert in (False, True):
        base = sr.pattern(n16, seed) ^ np.uint32(0xFFFFFFFF if invert else 0)
        bad = injected(base, n16, launched(n16, grid))
        for down in (False, True):
            for write in (False, True):
                what = (shape, invert, down, write)
                # clean: no error, and with the write an output complemented exactly once: one visit per slot
                got = hip.hbm_march_pass(base, seed, invert, down, write, grid=grid)
                compare(got, hc.march_pass(base, seed, invert, down, write), what)
                assert got["errors"] == 0 and np.array_equal(got["words"], ~base if write else base), what
                got = hip.hbm_march_pass(bad, seed, invert, down, write, grid=grid)
                want = hc.march_pass(bad, seed, invert, down, write)
                assert want["errors"] == int((bad != base).sum()) >= min(4 * n16, 4)
                compare(got, want, what)


def test_march_pass_against_the_other_seed_counts_every_word_and_drops_records():
    """More errors than records: the counters stay exact, 64 records are kept and the rest is reported."""
    from amdkube.ops import hip
    n16 = 7000
    words = sr.pattern(n16, SEEDS[0])
    want = hc.march_pass(words, SEEDS[1], False, True, True)
    got = hip.hbm_march_pass(words, SEEDS[1], False, True, True, grid=3)
    assert want["errors"] >= 4 * n16 - 1
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert len(got["records"]) == hc.RECORDS and got["records_dropped"] == want["errors"] - hc.RECORDS
    assert record_set(got["records"]) <= want["records"] and len(record_set(got["records"])) == hc.RECORDS
    assert np.array_equal(got["words"], want["words"]) and got["page_errors"].tolist() == [want["errors"]]


def test_march_pass_refuses_bad_grids_and_sizes():
    from amdkube.ops import hip
    words = np.zeros(4, np.uint32)
    for grid in (-1, 65537):
        with pytest.raises(ValueError):
            hip.hbm_march_pass(words, SEEDS[0], False, False, False, grid=grid)
    for bad in (np.zeros(0, np.uint32), np.zeros(6, np.uint32)):
        with pytest.raises(ValueError):
            hip.hbm_march_pass(bad, SEEDS[0], False, False, False)
    assert hip.hbm_march_pass(sr.pattern(1, SEEDS[0]), SEEDS[0], False, True, True, grid=65536)["errors"] == 0


# ---------------------------------------------------------------------------- the whole check
def test_check_runs_three_chunks_clean():
    from amdkube.ops import hip
    r = hip.hbm_check(mib=48, chunk_mib=16, rounds=2)
    plan = hc.plan(hip.device_info(0)["total_mem"], 48, chunk_mib=16)
    assert r["ok"] and r["bytes"] == plan["bytes"] == 48 * MIB and r["chunks"] == plan["chunks"] == [16 * MIB] * 3
    assert {k: r[k] for k in COUNTS} == dict.fromkeys(COUNTS, 0) and r["records_dropped"] == 0
    assert r["first_errors"] == [] and r["bad_pages"] == [] and r["bad_pages_total"] == 0
    assert r["rounds"] == 2 and r["ms"] > 0 and r["alloc_ms"] >= 0 and r["march_gbps"] > 0


def test_check_refuses_what_the_plan_refuses():
    from amdkube.ops import hip
    for kw in ({"mib": 48, "free_fraction": 0.5}, {"mib": 1}, {"mib": -1}, {"free_fraction": 0.0}, {"free_fraction": 0.96},
               {"mib": 48, "chunk_mib": 3}, {"mib": 48, "rounds": 0}, {"mib": 48, "selftest_flips": 65},
               {"mib": 1 << 29}):                                  # 512 TiB: does not fit
        with pytest.raises(ValueError):
            hip.hbm_check(**kw)


@functools.lru_cache(maxsize=None)
def complemented_background(seed, n16):
    """What E2 expects in chunk 0 of round 0."""
    return ~hc.pattern(n16, hc.chunk_seed(seed, 0, 0))


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("flips", [1, 7, 64])
def test_selftest_flips_are_found_where_they_were_made(flips, seed):
    from amdkube.ops import hip
    chunk_bytes = 16 * MIB
    n16 = chunk_bytes // hc.SLOT_BYTES
    r = hip.hbm_check(mib=32, chunk_mib=16, seed=seed, selftest_flips=flips)
    assert not r["ok"] and r["chunks"] == [chunk_bytes] * 2
    assert (r["errors"], r["bit_errors"], r["persistent"], r["transient"], r["records_dropped"]) == (flips, flips, flips, 0, 0)
    slots = hc.flip_slots(seed, flips, n16)
    want = complemented_background(seed, n16)
    expected = set()
    for f, slot in enumerate(slots):
        word, bit = hc.flip_bit(seed, f)
        w = int(want[4 * slot + word])
        expected.add((0, 2, 0, slot, word, w ^ (1 << bit), w, w ^ (1 << bit)))
    got = {(e["round"], e["pass"], e["chunk"], e["slot"], e["word"], e["got"], e["want"], e["again"]) for e in r["first_errors"]}
    assert len(r["first_errors"]) == flips and got == expected
    for e in r["first_errors"]:
        assert 0 <= e["xcc"] < 8 and 0 <= e["cu"] < 16 and 0 <= e["se"] < 8
    pages = collections.Counter(hc.page_of(s, 0, chunk_bytes) for s in slots)
    assert r["bad_pages"] == [{"offset": p * hc.PAGE_BYTES, "chunk": 0, "errors": c} for p, c in sorted(pages.items())]
    assert r["bad_pages_total"] == len(pages) <= hc.BAD_PAGES


# ---------------------------------------------------------------------------- the program
KEYS = {"device", "uuid", "arch", "free_bytes", "bytes", "chunks", "rounds", "hold_ms", "ms", "alloc_ms", "march_gbps", "errors",
        "bit_errors", "transient", "persistent", "records_dropped", "bad_pages_total", "bad_pages", "first_errors"}


def _hbm_check(*args, env=None):
    r = subprocess.run([os.path.join(BIN, "hbm-check"), *args], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


def test_binary_clean_run_prints_the_documented_keys():
    rc, lines, r = _hbm_check("--mib", "48", "--chunk-mib", "16", "--rounds", "2", "--hold-ms", "1")
    assert rc == 0 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    assert set(d) == KEYS, sorted(set(d) ^ KEYS)
    assert d["bytes"] == 48 * MIB and d["chunks"] == [16 * MIB] * 3 and d["rounds"] == 2 and d["hold_ms"] == 1
    assert {k: d[k] for k in COUNTS} == dict.fromkeys(COUNTS, 0) and d["first_errors"] == [] and d["bad_pages"] == []
    assert d["march_gbps"] > 0 and d["ms"] > 0 and d["arch"].startswith("gfx950") and d["free_bytes"] > d["bytes"]


def test_binary_reports_selftest_flips_with_their_place():
    rc, lines, r = _hbm_check("--mib", "32", "--chunk-mib", "16", "--selftest-flips", "3")
    assert rc == 1 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    assert d["errors"] == d["bit_errors"] == d["persistent"] == 3 and len(d["first_errors"]) == 3
    slots = hc.flip_slots(0x5EED, 3, 16 * MIB // hc.SLOT_BYTES)
    for e in d["first_errors"]:
        assert set(e) == {"round", "pass", "chunk", "slot", "word", "offset", "got", "want", "again", "xcc", "se", "sh", "cu"}, e
        assert e["pass"] == 2 and e["slot"] in slots and e["offset"] == 16 * e["slot"] + 4 * e["word"]
    assert sum(p["errors"] for p in d["bad_pages"]) == 3


def test_binary_bad_arguments_exit_2_before_the_gpu():
    """With every GPU hidden a run that touched the device would end with 4, not 2."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for args in (("--mib", "48", "--free-fraction", "0.5"), ("--free-fraction", "0"), ("--mib", "-1"), ("--mib", "1"),
                 ("--free-fraction", "0.96"), ("--chunk-mib", "3"), ("--rounds", "0"), ("--selftest-flips", "65"), ("--mib",),
                 ("--bogus", "1")):
        rc, lines, r = _hbm_check(*args, env=env)
        assert rc == 2 and r.stdout == "" and r.stderr.startswith("hbm-check:"), (args, r.stdout, r.stderr)


def test_binary_free_fraction_tests_that_share_of_free_memory():
    rc, lines, r = _hbm_check("--free-fraction", "0.001")
    assert rc == 0 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    plan = hc.plan(d["free_bytes"], free_fraction=0.001)
    assert d["bytes"] == plan["bytes"] >= hc.PAGE_BYTES and d["chunks"] == plan["chunks"] and d["errors"] == 0
    assert 0 <= d["free_bytes"] * 0.001 - d["bytes"] < hc.PAGE_BYTES + 1
