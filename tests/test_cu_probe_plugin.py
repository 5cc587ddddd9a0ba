"""Device-plugin side of the per-CU probe: `cu` in `health_probe`, run against stub probe binaries
that log their arguments, on the fake backend (CPU tier)."""
import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from amdkube.smi.health import HEALTH_REASON_ATTR
from tests.conftest import run
from tests.probe_stubs import make_stubs, start as _start

HBM_ARGS, MFMA_ARGS, LP_ARGS, CU_ARGS = "--mib 512 --iters 2", "--ms 200", "--dtype fp8,mxfp8,mxfp4 --ms 200", "--ms 200"


@pytest.fixture
def stubs(short_tmp, monkeypatch):
    return make_stubs(short_tmp, monkeypatch, fields=3)


def test_the_cu_probe_sits_in_its_own_table_and_runs_last():
    assert list(amd.HEALTH_PROBES) == ["hbm", "mfma", "mfma-lp"]                   # unchanged
    assert amd.HEALTH_PROBES_CU == {"cu": ("cu-check", ["--ms", "200"])}
    assert list(amd.all_health_probes()) == ["hbm", "mfma", "mfma-lp", "cu"]
    assert "--require-coverage" not in amd.HEALTH_PROBES_CU["cu"][1]
    assert amd.parse_health_probe("cu") == ["cu"]
    assert amd.parse_health_probe("cu,hbm") == ["hbm", "cu"]
    assert amd.parse_health_probe("cu, mfma-lp ,hbm,mfma") == ["hbm", "mfma", "mfma-lp", "cu"]
    assert amd.parse_health_probe("none") == []
    with pytest.raises(ValueError) as e:
        amd.parse_health_probe("cu,foo")
    assert all(name in str(e.value) for name in ("hbm", "mfma", "mfma-lp", "cu", "'foo'"))


def test_cu_runs_cu_check_on_every_gpu(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "cu")
        try:
            assert calls() == [("cu-check", t, CU_ARGS) for t in tokens]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_all_four_run_in_order_per_gpu(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "cu,mfma-lp,hbm,mfma")        # the order given does not matter
        try:
            assert calls() == [c for t in tokens for c in (("hbm-probe", t, HBM_ARGS), ("mfma-check", t, MFMA_ARGS),
                                                           ("mfma-check", t, LP_ARGS), ("cu-check", t, CU_ARGS))]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_a_failing_cu_check_sets_a_sticky_probe_reason(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("cu-check", tokens[1])

    async def go():
        p = await _start(fb, short_tmp, "hbm,mfma,mfma-lp,cu")
        try:
            assert [c[0] for c in calls() if c[1] == tokens[1]] == ["hbm-probe", "mfma-check", "mfma-check", "cu-check"]
            devs = {d["ID"]: d for d in p.devices}
            assert devs[ids[0]]["health"] == "Healthy" and HEALTH_REASON_ATTR not in devs[ids[0]]["Attributes"]
            assert devs[ids[1]]["health"] == "Unhealthy"
            assert p.reasons[ids[1]].startswith("probe: cu-check failed rc=1"), p.reasons
            assert devs[ids[1]]["Attributes"][HEALTH_REASON_ATTR].startswith("probe_cu-check")
            p._check_health()                                         # sticky across health ticks
            assert {d["ID"]: d["health"] for d in p.devices}[ids[1]] == "Unhealthy"
        finally:
            await p.stop()
    run(go())


def test_a_failure_before_cu_ends_that_gpus_chain(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("hbm-probe", tokens[0])

    async def go():
        p = await _start(fb, short_tmp, "hbm,cu")
        try:
            assert calls() == [("hbm-probe", tokens[0], HBM_ARGS), ("hbm-probe", tokens[1], HBM_ARGS),
                               ("cu-check", tokens[1], CU_ARGS)]
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Unhealthy", ids[1]: "Healthy"}
        finally:
            await p.stop()
    run(go())


def test_cli_accepts_cu_in_any_list_over_the_four_probes():
    from amdkube.cmd.components import device_plugin_parser
    ap = device_plugin_parser()
    for spec in ("cu", "hbm,mfma,mfma-lp,cu", "cu,hbm", "none", "hbm,mfma"):
        assert ap.parse_args(["--health-probe", spec]).health_probe == spec
    for spec in ("foo", "cu,foo", "", "none,hbm", "none,cu"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--health-probe", spec])


def test_the_cu_check_image_exists():
    from amdkube.runtime.images import builtin_images
    images = builtin_images()
    assert images["amdkube/cu-check:latest"]["entrypoint"][0].endswith("/_native/bin/cu-check")
    assert images["amdkube/mfma-check:latest"]["entrypoint"][0].endswith("/_native/bin/mfma-check")
