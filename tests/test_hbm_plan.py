"""kernels/hbm_plan.h on CPU: the region of hbm-check, its chunks, the way from a chunk and slot back to
an offset and a page, the chunk seeds and the self-test's slots, through the stand-alone self-test built
plain and with ASan/UBSan. See native/hbm_plan_selftest.cpp for what it checks. The numpy transcription
(amdkube/ops/hbmcheck.py) is held against the same cases here."""
import os
import subprocess
import sys

import pytest

from amdkube.ops import hbmcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))

MIB, GIB = 1 << 20, 1 << 30


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


@pytest.mark.parametrize("binary", ["hbm-plan-selftest", "hbm-plan-selftest-asan"])
def test_hbm_plan_selftest(binary):
    r = subprocess.run([os.path.join(BIN, binary)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_the_numpy_plan_gives_the_cases_of_the_selftest():
    free = 288 * GIB
    assert hbmcheck.plan(free, 48, chunk_mib=16) == {"bytes": 48 * MIB, "chunk_bytes": 16 * MIB, "chunks": [16 * MIB] * 3}
    assert hbmcheck.plan(free, 2500)["chunks"] == [GIB, GIB, 452 * MIB]
    assert hbmcheck.plan(free, 3)["bytes"] == 2 * MIB
    assert hbmcheck.plan(free, free_fraction=0.5)["bytes"] == 144 * GIB
    p = hbmcheck.plan(287 * GIB + 12345678, free_fraction=0.001)
    assert 0 <= (287 * GIB + 12345678) // 1000 - p["bytes"] < 2 * MIB + 1 and p["bytes"] % (2 * MIB) == 0
    for kw in ({}, {"mib": 48, "free_fraction": 0.5}, {"mib": -1}, {"mib": 1}, {"free_fraction": 0.96},
               {"free_fraction": -0.5}, {"mib": 48, "chunk_mib": 3}, {"mib": 48, "chunk_mib": 65538}, {"mib": 288 * 1024}):
        with pytest.raises(ValueError):
            hbmcheck.plan(free, **kw)
    assert hbmcheck.page_of(131071) == 0 and hbmcheck.page_of(131072) == 1
    assert hbmcheck.page_of(0, chunk=2, chunk_bytes=16 * MIB) == 16
