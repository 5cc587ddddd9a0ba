"""Device-plugin side of the low-precision matrix-core probe: `mfma-lp` in `health_probe`, run
against stub probe binaries that log their arguments, on the fake backend (CPU tier)."""
import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from amdkube.smi.health import HEALTH_REASON_ATTR
from tests.conftest import run
from tests.probe_stubs import make_stubs, start as _start

LP_ARGS = "--dtype fp8,mxfp8,mxfp4 --ms 200"


@pytest.fixture
def stubs(short_tmp, monkeypatch):
    return make_stubs(short_tmp, monkeypatch, fields=3)


def test_the_probe_table_keeps_its_order_and_gains_mfma_lp():
    assert list(amd.HEALTH_PROBES) == ["hbm", "mfma", "mfma-lp"]
    assert amd.HEALTH_PROBES["mfma-lp"] == ("mfma-check", ["--dtype", "fp8,mxfp8,mxfp4", "--ms", "200"])
    assert amd.HEALTH_PROBES["mfma"] == ("mfma-check", ["--ms", "200"])
    assert amd.parse_health_probe("mfma-lp") == ["mfma-lp"]
    assert amd.parse_health_probe("mfma-lp, hbm ,mfma") == ["hbm", "mfma", "mfma-lp"]


def test_mfma_lp_runs_mfma_check_with_the_dtype_list(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "mfma-lp")
        try:
            assert calls() == [("mfma-check", t, LP_ARGS) for t in tokens]
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_all_three_run_in_order_per_gpu_and_a_failure_ends_that_gpus_chain(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("mfma-check --ms 200", tokens[0])                            # the bf16 check fails on GPU 0

    async def go():
        p = await _start(fb, short_tmp, "mfma-lp,hbm,mfma")           # the order given does not matter
        try:
            assert calls() == [("hbm-probe", tokens[0], "--mib 512 --iters 2"), ("mfma-check", tokens[0], "--ms 200"),
                               ("hbm-probe", tokens[1], "--mib 512 --iters 2"), ("mfma-check", tokens[1], "--ms 200"),
                               ("mfma-check", tokens[1], LP_ARGS)]
            assert p.reasons[ids[0]].startswith("probe: mfma-check failed rc=1")
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Unhealthy", ids[1]: "Healthy"}
        finally:
            await p.stop()
    run(go())


def test_a_failing_mfma_lp_sets_a_sticky_probe_reason(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("--dtype", tokens[1])                                        # only the low-precision run fails, on GPU 1

    async def go():
        p = await _start(fb, short_tmp, "hbm,mfma,mfma-lp")
        try:
            assert [c[2] for c in calls() if c[1] == tokens[1]] == ["--mib 512 --iters 2", "--ms 200", LP_ARGS]
            devs = {d["ID"]: d for d in p.devices}
            assert devs[ids[0]]["health"] == "Healthy" and HEALTH_REASON_ATTR not in devs[ids[0]]["Attributes"]
            assert devs[ids[1]]["health"] == "Unhealthy"
            assert p.reasons[ids[1]].startswith("probe: mfma-check failed rc=1"), p.reasons
            assert devs[ids[1]]["Attributes"][HEALTH_REASON_ATTR].startswith("probe_mfma-check")
            p._check_health()                                         # sticky across health ticks
            assert {d["ID"]: d["health"] for d in p.devices}[ids[1]] == "Unhealthy"
        finally:
            await p.stop()
    run(go())


def test_cli_accepts_every_list_over_the_known_probes():
    from amdkube.cmd.components import device_plugin_parser
    ap = device_plugin_parser()
    assert ap.parse_args([]).health_probe == "none"
    for spec in ("none", "hbm", "mfma", "hbm,mfma", "mfma-lp", "hbm,mfma,mfma-lp", "mfma-lp,hbm"):
        assert ap.parse_args(["--health-probe", spec]).health_probe == spec
    for spec in ("foo", "hbm,foo", "", "none,hbm"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--health-probe", spec])
