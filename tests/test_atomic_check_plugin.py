"""Device-plugin side of the atomic-unit check: `atomic_check_ms` / `--atomic-check-ms`, run against stub
probe binaries that log their arguments, on the fake backend (CPU tier). The check is no entry of the probe
tables: it follows the `--health-probe` list and `--mfma-check-dtype`, precedes the HBM march, or runs alone
with `none`."""
import stat

import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from tests.conftest import run
from tests.probe_stubs import STUB, make_stubs, start as _start


@pytest.fixture
def stubs(short_tmp, monkeypatch):
    """make_stubs, with stubs of atomic-check and hbm-check beside the three it writes."""
    make3, calls = make_stubs(short_tmp, monkeypatch, fields=3)

    def make(fail="", fail_token=""):
        make3(fail, fail_token)
        for name in ("atomic-check", "hbm-check"):
            p = short_tmp / "bin" / name
            p.write_text(STUB.format(name=name, log=short_tmp / "probe.log", fail=fail, fail_token=fail_token))
            p.chmod(p.stat().st_mode | stat.S_IXUSR)
    return make, calls


@pytest.mark.parametrize("probe, kw, chain", [
    ("hbm,mfma,cu", dict(mfma_check_dtype="fp64,int8", atomic_check_ms=150, hbm_check_mib=512),
     [("hbm-probe", "--mib 512 --iters 2"), ("mfma-check", "--ms 200"), ("cu-check", "--ms 200"),
      ("mfma-check", "--dtype fp64,int8 --ms 200"), ("atomic-check", "--ms 150"), ("hbm-check", "--mib 512")]),
    ("none", dict(atomic_check_ms=200), [("atomic-check", "--ms 200")]),
    ("hbm", dict(), [("hbm-probe", "--mib 512 --iters 2")]),
])
def test_the_calls_per_gpu_and_their_order(short_tmp, stubs, probe, kw, chain):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)

    async def go():
        p = await _start(fb, short_tmp, probe, **kw)
        try:
            assert calls() == [(b, visibility_token(g), args) for g in fb.gpus() for b, args in chain]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_a_failing_atomic_check_sets_a_sticky_probe_reason(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("atomic-check", tokens[1])

    async def go():
        p = await _start(fb, short_tmp, "none", atomic_check_ms=100, hbm_check_mib=64)
        try:
            assert [c[0] for c in calls() if c[1] == tokens[1]] == ["atomic-check"]   # its chain ends there
            assert p.reasons[ids[1]].startswith("probe: atomic-check failed rc=1"), p.reasons
            p._check_health()                                                         # sticky across health ticks
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Healthy", ids[1]: "Unhealthy"}
        finally:
            await p.stop()
    run(go())


def test_the_parser_the_constructor_and_the_image():
    from amdkube.cmd.components import device_plugin_parser
    from amdkube.runtime.images import builtin_images
    ap = device_plugin_parser()
    assert ap.parse_args([]).atomic_check_ms == 0
    assert ap.parse_args(["--atomic-check-ms", "200"]).atomic_check_ms == 200
    for bad in ("-1", "x"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--atomic-check-ms", bad])
    with pytest.raises(ValueError):
        amd.AMDGPUPlugin(FakeBackend(n=1), atomic_check_ms=-1)
    assert builtin_images()["amdkube/atomic-check:latest"]["entrypoint"][0].endswith("/_native/bin/atomic-check")
