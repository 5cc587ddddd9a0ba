"""GPU tier: the lane check (kernels/lane_check.h: the DPP network and lane swaps, the LDS crossbar as a permute
unit, the transposing LDS reads, the direct global-to-LDS loads) through lane-check and the in-process ops.

Every operation is a pure permutation of hashed 32-bit words, so the oracle (amdkube/ops/lanecheck.py, written
from the headers' formulas) is exact and every comparison is bit for bit. One workgroup is the smallest shape
at which everything can go wrong: it holds all 16 waves, every control, all four transpose forms and all three
direct-load widths with the offset chunk; the first and the last workgroup of the grid are dumped. The plugin
option is tested against stub binaries (test_lane_check_plugin.py); LocalCluster passes no plugin options
through, so there is no cluster test here."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
SEED = 0x5EED
UNITS = ("dpp", "perm", "tr", "dma")
KEYS = {"device", "uuid", "arch", "units", "blocks", "rounds", "launches", "ms", "xlane_gops", "tr_gbps", "dma_gbps",
        "cus", "cus_covered", "simds", "simds_covered", "xccs", "errors", "errors_by_unit", "bad_cus", "first_errors"}
RECORD = {"unit", "block", "xcc", "se", "sh", "cu", "simd", "round", "op", "lane", "got", "want"}


def _lane_check(*args):
    r = subprocess.run([os.path.join(BIN, "lane-check"), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


def test_binary_clean_run_flips_and_bad_arguments():
    rc, lines, r = _lane_check("--rounds", "3", "--require-coverage")
    assert rc == 0 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    assert set(d) == KEYS, sorted(set(d) ^ KEYS)
    assert d["errors"] == 0 and d["first_errors"] == [] and d["bad_cus"] == [] and d["rounds"] == 3
    assert d["errors_by_unit"] == dict.fromkeys(UNITS, 0) and d["units"] == list(UNITS)
    assert d["blocks"] == 4 * d["cus"] and d["cus_covered"] == d["cus"] and d["simds_covered"] == d["simds"] == 4 * d["cus"]
    assert min(d["xlane_gops"], d["tr_gbps"], d["dma_gbps"], d["ms"]) > 0 and d["arch"].startswith("gfx950")
    rc, lines, r = _lane_check("--rounds", "2", "--selftest-flips", "5")
    assert rc == 1 and lines[0]["errors"] == 5 and len(lines[0]["first_errors"]) == 5, (r.stdout, r.stderr)
    assert all(set(e) == RECORD for e in lines[0]["first_errors"])
    for args in (("--units", "foo"), ("--units", "dpp,"), ("--selftest-flips", "5000"), ("--rounds", "0"), ("--ms",),
                 ("--bogus", "1")):
        rc, lines, r = _lane_check(*args)
        assert rc == 2 and r.stdout == "" and r.stderr.startswith("lane-check:"), (args, r.stdout, r.stderr)


@pytest.fixture(scope="module")
def blocks():
    from amdkube.ops import hip
    return 4 * hip.device_info()["cu_count"]


@pytest.fixture(scope="module")
def dumps(blocks):
    from amdkube.ops import hip
    return {blk: hip.lane_check_dump(blk, seed=SEED) for blk in (0, blocks - 1)}


@pytest.mark.parametrize("unit", UNITS)
def test_dump_equals_the_reference_bit_for_bit(dumps, unit):
    import numpy as np
    from amdkube.ops import lanecheck as lc
    ref = {"dpp": lc.dpp_table, "perm": lc.perm_table, "tr": lc.tr_registers, "dma": lc.dma_image}[unit]
    for blk, d in dumps.items():
        want = ref(SEED, blk)
        assert d[unit].dtype == np.uint32 and d[unit].shape == want.shape
        bad = np.argwhere(d[unit] != want)
        assert len(bad) == 0, (blk, len(bad), bad[:8].tolist())
        assert sorted(lc.decode_location(h, d["xcc_id"])["simd"] for h in d["hw_id"]) == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    assert not np.array_equal(*(d[unit] for d in dumps.values()))


def test_clean_run_and_unit_selection(blocks):
    from amdkube.ops import hip
    r = hip.lane_check(rounds=2)
    print("lane_check clean run:", {k: r[k] for k in ("ms", "xlane_gops", "tr_gbps", "dma_gbps", "simds_covered", "launches")})
    assert r["ok"] is True and r["errors"] == 0 and r["errors_by_unit"] == dict.fromkeys(UNITS, 0) and r["first_errors"] == []
    assert r["blocks"] == blocks == 4 * r["cus"] and r["cus_covered"] == r["cus"] and r["simds_covered"] == r["simds"]
    assert r["block_loc"].shape == (blocks, 17)
    r = hip.lane_check(rounds=2, units="tr")
    assert r["units"] == ["tr"] and r["errors"] == 0 and r["tr_gbps"] > 0 and r["xlane_gops"] == 0 and r["dma_gbps"] == 0
    with pytest.raises(ValueError):
        hip.lane_check(units="dpp,lds")
    with pytest.raises(ValueError):
        hip.lane_check_dump(blocks)                                   # outside the grid


@pytest.mark.parametrize("n, units", [(8, UNITS), (1, UNITS), (7, ("perm", "dma")), (100, UNITS)])
def test_selftest_flips_are_reported_where_the_host_put_them(blocks, n, units):
    from amdkube.ops import hip, lanecheck as lc
    r = hip.lane_check(rounds=2, selftest_flips=n, units=",".join(units))
    want = lc.flip_positions(SEED, n, blocks, units)
    assert r["errors"] == n and r["ok"] is False
    assert r["errors_by_unit"] == {u: sum(w[0] == u for w in want) for u in UNITS}
    assert len(r["first_errors"]) == min(n, 16)
    for e in r["first_errors"]:
        assert (e["unit"], e["block"], e["lane"]) in want, e
        x = e["got"] ^ e["want"]
        assert x != 0 and x & (x - 1) == 0 and e["round"] in (0, 1), e           # a single bit
        place = lc.decode_location(int(r["block_loc"][e["block"]][e["lane"] // 64 if e["unit"] != "dma" else 0]),
                                   int(r["block_loc"][e["block"]][16]))
        if e["unit"] == "dma":
            place.pop("simd")                                                    # read back by another wave
        assert place == {k: e[k] for k in place}, e
    if n <= 16:
        assert {(e["unit"], e["block"], e["lane"]) for e in r["first_errors"]} == set(want)
        assert sum(b["errors"] for b in r["bad_cus"]) == n
