"""Device-plugin side of the lane check: `lane_check_ms` / `--lane-check-ms`, run against stub probe binaries
that log their arguments, on the fake backend (CPU tier). The check is no entry of the probe tables: it follows
the `--health-probe` list, `--mfma-check-dtype` and `--atomic-check-ms`, precedes the HBM march, or runs alone
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
    """make_stubs, with stubs of atomic-check, lane-check and hbm-check beside the three it writes."""
    make3, calls = make_stubs(short_tmp, monkeypatch, fields=3)

    def make(fail="", fail_token=""):
        make3(fail, fail_token)
        for name in ("atomic-check", "lane-check", "hbm-check"):
            p = short_tmp / "bin" / name
            p.write_text(STUB.format(name=name, log=short_tmp / "probe.log", fail=fail, fail_token=fail_token))
            p.chmod(p.stat().st_mode | stat.S_IXUSR)
    return make, calls


@pytest.mark.parametrize("probe, kw, chain", [
    ("hbm,cu", dict(atomic_check_ms=150, lane_check_ms=120, hbm_check_mib=512),
     [("hbm-probe", "--mib 512 --iters 2"), ("cu-check", "--ms 200"), ("atomic-check", "--ms 150"),
      ("lane-check", "--ms 120"), ("hbm-check", "--mib 512")]),
    ("none", dict(lane_check_ms=200), [("lane-check", "--ms 200")]),
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


def test_a_failing_lane_check_sets_a_sticky_probe_reason(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("lane-check", tokens[1])

    async def go():
        p = await _start(fb, short_tmp, "none", lane_check_ms=100, hbm_check_mib=64)
        try:
            assert [c[0] for c in calls() if c[1] == tokens[1]] == ["lane-check"]     # its chain ends there
            assert p.reasons[ids[1]].startswith("probe: lane-check failed rc=1"), p.reasons
            p._check_health()                                                         # sticky across health ticks
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Healthy", ids[1]: "Unhealthy"}
        finally:
            await p.stop()
    run(go())


def test_the_parser_the_constructor_and_the_image():
    from amdkube.cmd.components import device_plugin_parser
    from amdkube.runtime.images import builtin_images
    ap = device_plugin_parser()
    assert ap.parse_args([]).lane_check_ms == 0
    assert ap.parse_args(["--lane-check-ms", "200"]).lane_check_ms == 200
    for bad in ("-1", "x", "1.5"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--lane-check-ms", bad])
    with pytest.raises(ValueError):
        amd.AMDGPUPlugin(FakeBackend(n=1), lane_check_ms=-1)
    assert amd.LANE_CHECK_TIMEOUT_S == amd.ATOMIC_CHECK_TIMEOUT_S == 60
    assert builtin_images()["amdkube/lane-check:latest"]["entrypoint"][0].endswith("/_native/bin/lane-check")
