"""native/io_trace.h on CPU: the I/O trace of hsa-vector-add through a stand-alone program's own
fopen / fclose / open / opendir, built plain, with ASan/UBSan and with ThreadSanitizer (two threads
opening files inside the window). See native/io_trace_selftest.cpp for what it checks."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))

VARIANTS = ["io-trace-selftest", "io-trace-selftest-asan", "io-trace-selftest-tsan"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


def selftest(binary, *args):
    r = subprocess.run([os.path.join(BIN, binary), *args], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


@pytest.mark.parametrize("binary", VARIANTS)
def test_io_trace_selftest(binary):
    r = selftest(binary)
    assert r.stdout.startswith("OK"), r.stdout + r.stderr[-3000:]


@pytest.mark.parametrize("binary", VARIANTS)
def test_path_lines(binary):
    assert selftest(binary, "paths").stderr.splitlines() == [
        "[path] fopen /proc/self/stat ok",
        "[path] fopen /nonexistent-io-trace/file No such file or directory",
        "[path] opendir /proc/self",
        "[path] opendir /nonexistent-io-trace/file",
    ]
