"""Device-plugin side of the HBM march: `hbm_check_mib` / `--hbm-check-mib`, run against stub probe binaries
that log their arguments, on the fake backend (CPU tier). The march is no entry of the probe tables: it
follows the `--health-probe` list, or runs alone with `none`."""
import stat

import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from amdkube.smi.health import HEALTH_REASON_ATTR
from tests.conftest import run
from tests.probe_stubs import STUB, make_stubs, start as _start

HBM_ARGS, CU_ARGS = "--mib 512 --iters 2", "--ms 200"


@pytest.fixture
def stubs(short_tmp, monkeypatch):
    """make_stubs, with a stub hbm-check beside the three it writes."""
    make3, calls = make_stubs(short_tmp, monkeypatch, fields=3)

    def make(fail="", fail_token=""):
        make3(fail, fail_token)
        p = short_tmp / "bin" / "hbm-check"
        p.write_text(STUB.format(name="hbm-check", log=short_tmp / "probe.log", fail=fail, fail_token=fail_token))
        p.chmod(p.stat().st_mode | stat.S_IXUSR)
    return make, calls


def test_the_probe_tables_are_what_they_were():
    assert list(amd.all_health_probes()) == ["hbm", "mfma", "mfma-lp", "cu"]
    assert not any(binary == "hbm-check" for binary, _ in amd.all_health_probes().values())
    with pytest.raises(ValueError):
        amd.parse_health_probe("hbm-check")


def test_flag_off_means_no_call(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        for probe in ("none", "hbm"):
            p = await _start(fb, short_tmp, probe)
            try:
                assert p.hbm_check_mib == 0
            finally:
                await p.stop()
        assert calls() == [("hbm-probe", t, HBM_ARGS) for t in tokens]
    run(go())


def test_flag_on_runs_one_hbm_check_per_gpu_after_the_list(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "cu,hbm", hbm_check_mib=4096)
        try:
            assert calls() == [c for t in tokens for c in (("hbm-probe", t, HBM_ARGS), ("cu-check", t, CU_ARGS),
                                                           ("hbm-check", t, "--mib 4096"))]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_flag_on_runs_with_none_too(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "none", hbm_check_mib=512)
        try:
            assert calls() == [("hbm-check", t, "--mib 512") for t in tokens]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_a_failing_hbm_check_sets_a_sticky_probe_reason(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("hbm-check", tokens[1])

    async def go():
        p = await _start(fb, short_tmp, "hbm", hbm_check_mib=2048)
        try:
            assert [c[0] for c in calls() if c[1] == tokens[1]] == ["hbm-probe", "hbm-check"]
            devs = {d["ID"]: d for d in p.devices}
            assert devs[ids[0]]["health"] == "Healthy" and HEALTH_REASON_ATTR not in devs[ids[0]]["Attributes"]
            assert devs[ids[1]]["health"] == "Unhealthy"
            assert p.reasons[ids[1]].startswith("probe: hbm-check failed rc=1"), p.reasons
            assert devs[ids[1]]["Attributes"][HEALTH_REASON_ATTR].startswith("probe_hbm-check")
            p._check_health()                                         # sticky across health ticks
            assert {d["ID"]: d["health"] for d in p.devices}[ids[1]] == "Unhealthy"
        finally:
            await p.stop()
    run(go())


def test_an_earlier_probe_failure_skips_the_hbm_check(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("hbm-probe", tokens[0])

    async def go():
        p = await _start(fb, short_tmp, "hbm", hbm_check_mib=2048)
        try:
            assert calls() == [("hbm-probe", tokens[0], HBM_ARGS), ("hbm-probe", tokens[1], HBM_ARGS),
                               ("hbm-check", tokens[1], "--mib 2048")]
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Unhealthy", ids[1]: "Healthy"}
            assert p.reasons[ids[0]].startswith("probe: hbm-probe failed rc=1")
        finally:
            await p.stop()
    run(go())


def test_the_time_limit_grows_with_the_size():
    assert amd.hbm_check_timeout(0) == amd.HBM_CHECK_BASE_S
    assert amd.hbm_check_timeout(8192) == amd.HBM_CHECK_BASE_S + 8 * amd.HBM_CHECK_S_PER_GIB
    assert amd.hbm_check_timeout(262144) > amd.hbm_check_timeout(8192) > amd.HBM_CHECK_BASE_S > 0


def test_the_parser_takes_a_size_and_refuses_a_negative_one():
    from amdkube.cmd.components import device_plugin_parser
    ap = device_plugin_parser()
    assert ap.parse_args([]).hbm_check_mib == 0
    assert ap.parse_args(["--hbm-check-mib", "8192"]).hbm_check_mib == 8192
    assert ap.parse_args(["--hbm-check-mib", "0", "--health-probe", "none"]).hbm_check_mib == 0
    for bad in ("-1", "-4096", "many", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(["--hbm-check-mib", bad])
    with pytest.raises(ValueError):
        amd.AMDGPUPlugin(FakeBackend(n=1), hbm_check_mib=-1)


def test_the_hbm_check_image_exists():
    from amdkube.runtime.images import builtin_images
    images = builtin_images()
    assert images["amdkube/hbm-check:latest"]["entrypoint"][0].endswith("/_native/bin/hbm-check")
    assert images["amdkube/hbm-probe:latest"]["entrypoint"][0].endswith("/_native/bin/hbm-probe")
