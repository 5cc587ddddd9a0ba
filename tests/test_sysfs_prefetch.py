"""native/sysfs_prefetch.h on CPU: the self-test on a fake KFD topology tree, through the program's
own interposed fopen, built plain, with ASan/UBSan and with ThreadSanitizer (readers racing the
helper thread). See native/sysfs_prefetch_selftest.cpp for what it checks."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))

VARIANTS = ["sysfs-prefetch-selftest", "sysfs-prefetch-selftest-asan", "sysfs-prefetch-selftest-tsan"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


def selftest(binary, *args, **env):
    r = subprocess.run([os.path.join(BIN, binary), *args], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", **env))
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("binary", VARIANTS)
def test_prefetch_selftest(binary):
    assert "prefetch=on" in selftest(binary)


@pytest.mark.parametrize("binary", VARIANTS)
def test_prefetch_switched_off_by_flag(binary):
    assert "prefetch=off" in selftest(binary, "--no-prefetch")


def test_prefetch_switched_off_by_environment():
    assert "prefetch=off" in selftest("sysfs-prefetch-selftest", AMDKUBE_VADD_PREFETCH="0")
    assert "prefetch=on" in selftest("sysfs-prefetch-selftest", AMDKUBE_VADD_PREFETCH="1")
