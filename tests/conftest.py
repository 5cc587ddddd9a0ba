import asyncio
import gc
import logging
import os
import pathlib
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run via gpurun)")
    config.addinivalue_line("markers", "slow: long-running test")
    config.addinivalue_line("markers", "needs_root(net=False): mounts or namespaces that take root; an ordinary user "
                                       "runs the test as root of a user namespace of its own")
    # native artefacts are not versioned: (re)build whatever is missing or stale (no-op when fresh)
    from native import build as nb
    nb.build(sanitize=True)


# Shutdown hygiene: every component's stop() awaits its tasks and closes its sessions. asyncio
# reports a leak through its logger (the loop's default exception handler); any such report
# during a test fails it.
_LEAK_MARKS = ("Task was destroyed but it is pending", "Unclosed client session", "Unclosed connector")


class _LeakRecorder(logging.Handler):
    def __init__(self):
        super().__init__(logging.ERROR)
        self.seen: list[str] = []

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith(_LEAK_MARKS):
            self.seen.append(msg.splitlines()[0] + " " + " ".join(msg.splitlines()[1:2])[:200])


_LEAKS = _LeakRecorder()
logging.getLogger("asyncio").addHandler(_LEAKS)


@pytest.fixture(autouse=True)
def no_leaked_tasks_or_sessions():
    _LEAKS.seen.clear()
    yield
    gc.collect()
    if _LEAKS.seen:
        found, _LEAKS.seen[:] = list(_LEAKS.seen), []
        pytest.fail("asyncio leak (a stop() that does not await its tasks or close its sessions):\n  " + "\n  ".join(found))


def run(coro, timeout=60):
    """Run a coroutine to completion on a fresh event loop (no pytest-asyncio here)."""
    return asyncio.run(asyncio.wait_for(coro, timeout))


def log_text(path: str) -> str:
    """A container's output from its log file (the CRI records the log pump writes, decoded)."""
    from amdkube.kubelet.logs import read_text
    return read_text(path)


@pytest.fixture
def short_tmp():
    """A scratch directory with a short path, for tests that bind unix sockets beneath it: a
    socket address holds 107 bytes, and pytest's tmp_path under a long TMPDIR exceeds that."""
    d = tempfile.mkdtemp(prefix="ak-", dir="/tmp")
    yield pathlib.Path(d)
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def arun():
    return run


# A `needs_root` test run by an ordinary user: the same test, run by a child pytest that is root
# in a user namespace (with mount and pid namespaces of its own, and with net=True a network
# namespace whose loopback is up). Where the kernel gives this user no user namespace it skips.
_USERNS_BOOT = """
import sys
if sys.argv[3] == "net":
    import fcntl, socket, struct
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    flags = struct.unpack("16sH22x", fcntl.ioctl(s, 0x8913, struct.pack("16sH22x", b"lo", 0)))[1]    # SIOCGIFFLAGS
    fcntl.ioctl(s, 0x8914, struct.pack("16sH22x", b"lo", flags | 1))                                   # SIOCSIFFLAGS, IFF_UP
    s.close()
import pytest
sys.exit(pytest.main(["-q", "-x", "-p", "no:cacheprovider", "--basetemp", sys.argv[2], sys.argv[1]]))
"""


def _unshare(net: bool) -> list[str]:
    return ["unshare", "--user", "--map-root-user", "--mount", "--pid", "--fork", "--mount-proc"] + (["--net"] if net else [])


def _run_in_userns(item, net: bool):
    import subprocess
    try:
        ok = subprocess.run(_unshare(net) + ["true"], capture_output=True, timeout=30).returncode == 0
    except (OSError, subprocess.SubprocessError):
        ok = False
    if not ok:
        pytest.skip("needs root, or a kernel that lets this user create user namespaces")
    base = tempfile.mkdtemp(prefix="ak-", dir="/tmp")
    try:
        r = subprocess.run(_unshare(net) + [sys.executable, "-c", _USERNS_BOOT, item.nodeid, os.path.join(base, "t"),
                                            "net" if net else "-"],
                           cwd=str(item.config.rootpath), capture_output=True, text=True, timeout=300)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    tail = r.stdout[-6000:] + r.stderr[-2000:]
    if r.returncode == 0 and " skipped" in r.stdout.strip().splitlines()[-1]:
        pytest.skip("skipped as root of a user namespace:\n" + tail)
    assert r.returncode == 0 and "1 passed" in r.stdout, tail


@pytest.hookimpl(tryfirst=True)
def pytest_pyfunc_call(pyfuncitem):
    """`async def test_*` runs on a fresh event loop with a 120 s cap."""
    mark = pyfuncitem.get_closest_marker("needs_root")
    if mark is not None and os.geteuid() != 0:
        _run_in_userns(pyfuncitem, bool(mark.kwargs.get("net")))
        return True
    if asyncio.iscoroutinefunction(pyfuncitem.obj):
        args = {k: pyfuncitem.funcargs[k] for k in pyfuncitem._fixtureinfo.argnames}
        run(pyfuncitem.obj(**args), timeout=120)
        return True
    return None
