"""kernels/vadd_contract.h on CPU: the flags, inputs, verification, grid and output lines that
rocm-vector-add and hsa-vector-add share, through the stand-alone self-test built plain and with
ASan/UBSan. See native/vadd_contract_selftest.cpp for what it checks; among it, that the verification
counts a NaN (in c, from the 0xff fill, from a NaN input, from inf - inf) where the two loops it replaced did not."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


@pytest.mark.parametrize("binary", ["vadd-contract-selftest", "vadd-contract-selftest-asan"])
def test_vadd_contract_selftest(binary):
    r = subprocess.run([os.path.join(BIN, binary)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    assert "nan counts" in r.stdout, r.stdout     # a NaN difference is a mismatch: the cases ran
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
