"""hsa-vector-add with and without its prefetch of hsa_init's file reads (native/sysfs_prefetch.h),
on a real MI355X: the two modes must be indistinguishable in everything but time. The pod tests in
tests/test_gpu.py (test_02, test_02c, test_04b) cover the same binary behind the device guard."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
SIZES = [1, 3, 255, 1025, 50000]   # the workload's own size, and the ragged ones where the tail and 16-byte paths meet


def vadd(*args, binary="hsa-vector-add", **env):
    return subprocess.run([os.path.join(BIN, binary), *args], capture_output=True, text=True, timeout=60,
                          env=dict(os.environ, **env))


def identity(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("GPU 0:")]
    assert len(lines) == 1, stdout
    return lines[0]


def result(stdout):
    j = json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("{")))
    prefetch = j.pop("prefetch")
    j.pop("kernel_ms")
    return j, prefetch


@pytest.fixture(scope="module")
def hip_identity():
    r = vadd("--print-uuid", binary="rocm-vector-add")
    assert r.returncode == 0 and "Test PASSED" in r.stdout, r.stdout + r.stderr
    return identity(r.stdout)


@pytest.mark.parametrize("n", SIZES)
def test_both_modes_agree(n, hip_identity):
    on = vadd("--print-uuid", "--json", "-n", str(n))
    off = vadd("--print-uuid", "--json", "-n", str(n), "--no-prefetch")
    for r in (on, off):
        assert r.returncode == 0 and "Test PASSED" in r.stdout, r.stdout + r.stderr
    assert identity(on.stdout) == identity(off.stdout) == hip_identity
    j_on, p_on = result(on.stdout)
    j_off, p_off = result(off.stdout)
    assert j_on == j_off and j_on["ok"] is True and j_on["n"] == n
    assert p_on is True and p_off is False


@pytest.mark.parametrize("n", [1, 1025])   # the smallest size, and the smallest at which the two programs' grids differ
def test_hip_and_hsa_builds_print_the_same_lines(n):
    hip = vadd("-n", str(n), binary="rocm-vector-add")
    hsa = vadd("-n", str(n))
    for r in (hip, hsa):
        assert r.returncode == 0 and r.stdout.endswith("Test PASSED\n"), r.stdout + r.stderr
    assert hip.stdout.splitlines() == hsa.stdout.splitlines()
    assert len(hsa.stdout.splitlines()) == 3 and f"[Vector addition of {n} elements]" in hsa.stdout


def prefetch_trace(stderr):
    m = re.search(r"^\[trace\] prefetch (\S+) (.*)$", stderr, re.M)
    assert m, stderr
    return m.group(1), {k: float(v) for k, v in (p.split("=") for p in m.group(2).split())}


def test_trace_counts_hits_only_with_prefetch_on():
    on = vadd(AMDKUBE_VADD_TRACE="1")
    off = vadd("--no-prefetch", AMDKUBE_VADD_TRACE="1")
    env_off = vadd(AMDKUBE_VADD_TRACE="1", AMDKUBE_VADD_PREFETCH="0")
    for r in (on, off, env_off):
        assert r.returncode == 0 and "Test PASSED" in r.stdout, r.stdout + r.stderr
    state, c = prefetch_trace(on.stderr)
    print(on.stderr)
    assert state == "on" and c["hits"] > 0 and c["files"] > 0 and c["bytes"] > 0
    for r in (off, env_off):
        state, c = prefetch_trace(r.stderr)
        assert state == "off" and c["hits"] == 0 and c["files"] == 0
    # the phase table splits hsa_init at the /dev/kfd open, and has one line per I/O group
    for r in (on, off):
        assert re.search(r"^\[trace\] init:kfd-wait\s+[\d.]+ ms$", r.stderr, re.M), r.stderr
        assert re.search(r"^\[trace\] init:post-wait\s+[\d.]+ ms$", r.stderr, re.M), r.stderr
        assert re.search(r"^\[trace\] io kfd-topology\s+fopen=\d+ ", r.stderr, re.M), r.stderr


@pytest.mark.parametrize("mode", [(), ("--no-prefetch",)], ids=["prefetch", "no-prefetch"])
def test_expect_devices_still_exits_3(mode):
    r = vadd("--expect-devices", "2", *mode)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "expected 2 visible GPU(s), found 1" in r.stderr
