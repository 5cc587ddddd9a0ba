"""GPU tier: the per-CU check (kernels/cu_check.h: LDS march, vector ALU pipes, transcendental unit,
workgroup placement) through every layer: cu-check, the device plugin's cu probe and the in-process ops.

The tests that start child processes come first, as in test_gpu_mfma_check.py, and torch is not
needed here at all. The oracle is amdkube/ops/cucheck.py, written from the header's formulas.

Numerics. The LDS image and the four multiply-add forms are exact: the products stay below 2^24
(fp32) and 2^53 (fp64). The transcendental unit has no exact reference; its bound per instruction is
the largest error measured on an MI355X against the float64 numpy function rounded to fp32, over the
dumped blocks and two further seeds, plus one ulp (docs/PERFORMANCE.md has the measurements):
TRANS_ULP_BOUND below.
"""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

from amdkube.localcluster import LocalCluster  # noqa: E402
from tests.conftest import run  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
SEED = 0x5EED
# measured maximum (1 ulp for each of the five) + 1, in fp32 ulps of the float64 reference rounded to fp32
TRANS_ULP_BOUND = {"exp2": 2.0, "log2": 2.0, "rcp": 2.0, "rsq": 2.0, "sqrt": 2.0}
KEYS = {"device", "uuid", "arch", "units", "blocks", "rounds", "launches", "ms", "lds_gbps", "valu_gops", "cus",
        "cus_covered", "xccs", "errors", "errors_by_unit", "bad_cus", "first_errors"}


def _cu_check(*args):
    r = subprocess.run([os.path.join(BIN, "cu-check"), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


# ---------------------------------------------------------------- the binary and the plugin
def test_binary_clean_run_prints_the_documented_keys():
    rc, lines, r = _cu_check("--rounds", "2", "--require-coverage")
    assert rc == 0 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    assert set(d) == KEYS, sorted(set(d) ^ KEYS)
    assert d["errors"] == 0 and d["first_errors"] == [] and d["bad_cus"] == [] and d["rounds"] == 2
    assert d["errors_by_unit"] == {"lds": 0, "valu": 0, "trans": 0} and d["units"] == ["lds", "valu", "trans"]
    assert d["cus"] > 0 and d["cus_covered"] == d["cus"] and d["blocks"] == 4 * d["cus"] and 1 <= d["xccs"] <= 8
    assert d["lds_gbps"] > 0 and d["valu_gops"] > 0 and d["ms"] > 0 and d["arch"].startswith("gfx950")


def test_binary_reports_selftest_flips_with_a_place():
    rc, lines, r = _cu_check("--rounds", "2", "--selftest-flips", "5")
    assert rc == 1 and len(lines) == 1, (r.stdout, r.stderr)
    d = lines[0]
    assert d["errors"] == 5 and d["errors_by_unit"] == {"lds": 2, "valu": 2, "trans": 1} and len(d["first_errors"]) == 5
    assert sum(b["errors"] for b in d["bad_cus"]) == 5
    for e in d["first_errors"]:
        assert set(e) == {"unit", "block", "xcc", "se", "sh", "cu", "round", "pass", "index", "got", "want"}, e


def test_binary_unit_selection_and_bad_arguments():
    rc, lines, r = _cu_check("--rounds", "1", "--units", "trans,lds")
    assert rc == 0 and lines[0]["units"] == ["lds", "trans"] and lines[0]["valu_gops"] == 0, (r.stdout, r.stderr)
    for args in (("--units", "foo"), ("--units", "lds,foo"), ("--selftest-flips", "5000"), ("--rounds", "0"), ("--ms",),
                 ("--bogus", "1")):
        rc, lines, r = _cu_check(*args)
        assert rc == 2 and r.stdout == "" and r.stderr.startswith("cu-check:"), (args, r.stdout, r.stderr)


def test_plugin_cu_probe_marks_healthy():
    async def go():
        async with LocalCluster(gpus="amdsmi", n_gpus=1, with_controllers=False, health_probe="cu") as lc:
            node = await lc.wait_gpus(1, 120)
            devs = node["status"]["extendedResources"]["amd.com/gpu"]["resources"]
            assert devs and all(d["health"] == "Healthy" for d in devs.values()), lc.plugin.reasons
    run(go(), 300)


# ---------------------------------------------------------------- dumps against the host reference
@pytest.fixture(scope="module")
def blocks():
    from amdkube.ops import hip
    return 4 * hip.device_info()["cu_count"]


@pytest.fixture(scope="module")
def dumps(blocks):
    from amdkube.ops import hip
    return {blk: hip.cu_check_dump(blk, seed=SEED) for blk in (0, blocks - 1)}


def test_dump_lds_image_equals_the_pattern_word_for_word(dumps):
    import numpy as np
    from amdkube.ops import cucheck
    for blk, d in dumps.items():
        assert d["lds"].dtype == np.uint32 and d["lds"].shape == (40960,)
        assert np.array_equal(d["lds"], cucheck.lds_pattern(SEED, blk, 0, 1)), blk
    assert not np.array_equal(*(d["lds"] for d in dumps.values()))


def test_dump_valu_results_equal_the_exact_reference(dumps):
    import numpy as np
    from amdkube.ops import cucheck
    for blk, d in dumps.items():
        ops = cucheck.valu_operands(SEED, blk)
        assert np.array_equal(d["valu_ops"], ops), blk
        want = cucheck.valu_expected(ops)
        f32, f64, i64 = d["valu_f32"], d["valu_f64"], d["valu_int"].astype(np.int64)
        assert f32.dtype == np.float32 and f64.dtype == np.float64
        for form, got in (("fp32", f32[:, 0:2]), ("packed fp32", f32[:, 2:4]), ("fp64", f64[:, 0:2]), ("integer", i64[:, 0:2])):
            assert np.array_equal(got.astype(np.float64), want[:, 0:2].astype(np.float64)), (blk, form)
        assert np.array_equal(f64[:, 2], want[:, 2].astype(np.float64)) and np.array_equal(i64[:, 2], want[:, 2]), blk
        assert np.array_equal(i64[:, 3], want[:, 3]), blk


def _ulps(out, ref64):
    """|out - fl32(ref64)| in ulps of fl32(ref64)."""
    import numpy as np
    ref32 = ref64.astype(np.float32)
    return np.abs(out.astype(np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64)


def test_dump_trans_outputs_lie_within_the_measured_bound(dumps):
    import numpy as np
    from amdkube.ops import cucheck
    for blk, d in dumps.items():
        x = cucheck.trans_inputs(SEED, blk)
        assert np.array_equal(d["trans_in"].view(np.uint32), x.view(np.uint32)), blk
        err = _ulps(d["trans_out"], cucheck.trans_reference(x))
        for f, name in enumerate(cucheck.TRANS_FUNCS):
            worst = float(err[:, f].max())
            print(f"trans {name} block {blk}: max error {worst:.3f} ulp (bound {TRANS_ULP_BOUND[name]})")
            assert worst <= TRANS_ULP_BOUND[name], (blk, name, worst)
        out = d["trans_out"].reshape(16, 64, 5, 4)                     # a wave pair agrees bit for bit
        assert np.array_equal(out[0::2].view(np.uint32), out[1::2].view(np.uint32))


def test_dump_location_is_decoded_from_the_raw_words(dumps, blocks):
    from amdkube.ops import cucheck, hip
    for d in dumps.values():
        assert d["location"] == cucheck.decode_location(d["hw_id"], d["xcc_id"]) and d["location"]["xcc"] < 8
    with pytest.raises(ValueError):
        hip.cu_check_dump(blocks)                                     # outside the grid


# ---------------------------------------------------------------- runs
def _place(e):
    return (e["xcc"], e["se"], e["sh"], e["cu"])


def test_clean_run_covers_every_cu(blocks):
    from collections import Counter
    from amdkube.ops import hip
    r = hip.cu_check(rounds=3)
    print("cu_check clean run:", {k: r[k] for k in ("cus", "cus_covered", "xccs", "launches", "ms", "lds_gbps", "valu_gops")})
    assert r["ok"] is True and r["errors"] == 0 and r["first_errors"] == [] and r["bad_cus"] == []
    assert r["errors_by_unit"] == {"lds": 0, "valu": 0, "trans": 0}
    assert r["cus"] == hip.device_info()["cu_count"] and r["blocks"] == blocks and r["rounds"] == 3
    assert 1 <= r["launches"] <= 4
    assert r["cus_covered"] == r["cus"] == len(r["locations"]) == len({_place(x) for x in r["locations"]})
    per_xcc = Counter(x["xcc"] for x in r["locations"])
    assert len(per_xcc) == r["xccs"] and max(per_xcc) < 8
    assert set(per_xcc.values()) == {r["cus"] // r["xccs"]}, per_xcc
    assert r["block_loc"].shape == (blocks, 2)


@pytest.mark.parametrize("n", [1, 3, 100, 4096])
def test_selftest_flips_are_all_reported_with_their_place(blocks, n):
    from amdkube.ops import cucheck, hip
    r = hip.cu_check(rounds=2, selftest_flips=n)
    assert r["errors"] == n and r["ok"] is False, r["errors_by_unit"]
    assert r["errors_by_unit"] == {u: len(range(i, n, 3)) for i, u in enumerate(("lds", "valu", "trans"))}
    recs = r["first_errors"]
    assert len(recs) == min(n, 16)
    for e in recs:
        assert 0 <= e["block"] < blocks and e["round"] in (0, 1) and e["unit"] in ("lds", "valu", "trans"), e
        x = e["got"] ^ e["want"]
        assert x != 0 and x & (x - 1) == 0, e                         # a single bit
        raw = r["block_loc"][e["block"]]
        assert cucheck.decode_location(int(raw[0]), int(raw[1])) == {k: e[k] for k in ("xcc", "se", "sh", "cu")}, e
        if e["unit"] == "lds":
            assert e["pass"] in (2, 3, 4) and e["index"] % 4 == 0 and e["index"] < 163840, e
    assert sum(b["errors"] for b in r["bad_cus"]) == n if n <= 16 else len(r["bad_cus"]) == 16
    assert {_place(b) for b in r["bad_cus"]} <= {_place(x) for x in r["locations"]}


@pytest.mark.parametrize("unit", ["lds", "valu", "trans"])
def test_unit_selection_reports_every_flip_under_that_unit(unit):
    from amdkube.ops import hip
    r = hip.cu_check(rounds=2, selftest_flips=7, units=(unit,))
    assert r["units"] == [unit] and r["errors"] == 7
    assert r["errors_by_unit"] == {u: 7 if u == unit else 0 for u in ("lds", "valu", "trans")}
    assert {e["unit"] for e in r["first_errors"]} == {unit} and len(r["first_errors"]) == 7


def test_two_units_split_the_flips_between_them():
    from amdkube.ops import hip
    r = hip.cu_check(rounds=1, selftest_flips=9, units=("valu", "trans"))
    assert r["errors"] == 9 and r["errors_by_unit"] == {"lds": 0, "valu": 5, "trans": 4}
    assert {e["round"] for e in r["first_errors"]} == {0}
