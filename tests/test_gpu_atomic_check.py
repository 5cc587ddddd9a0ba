"""The atomic-unit check on the GPU (kernels/atomic_check.h): the tables one scatter launch leaves behind
against the numpy reference (amdkube/ops/atomiccheck.py), bit for bit: every op is order-independent by
construction, so there is no tolerance; a clean run and its checked count; the self-test's flips found at
their positions; and the atomic-check binary with its exit codes."""
import json
import os
import subprocess

import numpy as np
import pytest

from amdkube.ops import atomiccheck as ac

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")


# (4, 1024): S = 1, every lane on one address, the CAS op gated off; (4, 1): S = G; (4, 64): the largest
# contention with the CAS op; (1, 256): one workgroup, where the LDS and the global shapes coincide
@pytest.mark.parametrize("seed", (0x5EED, 0xC0FFEE))
@pytest.mark.parametrize("blocks, contention", [(4, 1), (4, 64), (4, 1024), (1, 256)])
def test_tables_equal_the_reference_bit_for_bit(blocks, contention, seed):
    from amdkube.ops import hip
    got = hip.atomic_check_tables(contention, blocks, seed=seed, round=1)
    want = ac.global_tables(blocks * ac.WG, contention, seed, 1)
    want["lds"] = ac.lds_tables(0, contention, seed, 1)
    assert set(got) == set(want) and set(got["lds"]) == set(want["lds"]) and ("cas_add" in got) == (contention <= 64)
    got["order"] = np.sort(got["order"], axis=1)          # per slot, the ids in any arrival order
    for where, g, w in [("", got, want), ("lds ", got["lds"], want["lds"])]:
        for op in (k for k in w if k != "lds"):
            assert g[op].dtype == w[op].dtype and g[op].shape == w[op].shape, where + op
            bad = np.flatnonzero((g[op].view(np.uint8) != w[op].view(np.uint8)).reshape(w[op].shape[0], -1).any(axis=1))
            assert bad.size == 0, f"{where}{op}: slots {bad[:8]} got {g[op][bad[:8]]} want {w[op][bad[:8]]}"


def test_a_clean_run_checks_the_closed_form_count():
    from amdkube.ops import hip
    r = hip.atomic_check(rounds=2)
    assert r["errors"] == 0 and r["ok"] and not r["first_errors"], r
    assert r["rounds"] == 2 and r["contention"] == list(ac.DEFAULT_CONTENTION) and r["blocks"] == ac.DEFAULT_BLOCKS
    assert r["checked"] == ac.checked_count(r["blocks"], r["contention"], 2) and r["atomics_per_s"] > 0


@pytest.mark.parametrize("n", (1, 7))
def test_selftest_flips_are_reported_at_their_positions(n):
    from amdkube.ops import hip
    r = hip.atomic_check(rounds=1, selftest_flips=n, blocks=4, contention=(64, 1))
    flipped = {(f["op"], f["slot"], f["contention"]) for f in r["selftest_positions"]}
    assert len(flipped) == n and r["errors"] == n and sum(r["errors_by_unit"].values()) == n, r
    assert {(e["op"], e["slot"], e["contention"]) for e in r["first_errors"]} == flipped
    assert all(e["got"] == e["want"] ^ 1 and e["round"] == 0 for e in r["first_errors"]), r["first_errors"]


def binary(*args):
    return subprocess.run([os.path.join(BIN, "atomic-check"), *args], capture_output=True, text=True, timeout=120)


def test_binary_clean_run_and_selftest():
    r = binary("--rounds", "2")
    out = json.loads(r.stdout)
    assert r.returncode == 0 and out["errors"] == 0 and out["rounds"] == 2 and out["units"] == list(ac.UNITS), r.stdout + r.stderr
    assert out["checked"] == ac.checked_count(out["blocks"], out["contention"], 2) and out["arch"].startswith("gfx")
    r = binary("--selftest-flips", "3", "--rounds", "1")
    out = json.loads(r.stdout)
    assert r.returncode == 1 and out["errors"] == 3 and len(out["first_errors"]) == 3, r.stdout + r.stderr


@pytest.mark.parametrize("args", [("--frobnicate", "1"), ("--units", "foo"), ("--contention", "3"), ("--rounds",)])
def test_binary_refuses_bad_arguments_before_the_gpu(args):
    r = binary(*args)
    assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("atomic-check:"), r
