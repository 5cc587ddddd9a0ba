"""Device-plugin side of the matrix-core health probe: `health_probe` as a comma list over hbm and
mfma, run against stub probe binaries on the fake backend (CPU tier)."""
import os

import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from amdkube.smi.health import HEALTH_REASON_ATTR, request_reset
from tests.conftest import run
from tests.probe_stubs import make_stubs, start as _start


@pytest.fixture
def stubs(short_tmp, monkeypatch):
    return make_stubs(short_tmp, monkeypatch, fields=2)


def test_mfma_probe_marks_the_failing_gpu_and_a_reset_clears_it(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    assert tokens[0] != tokens[1]
    make("mfma-check", tokens[1])
    state = str(short_tmp / "health.json")

    async def go():
        p = await _start(fb, short_tmp, "mfma", health_state=state)
        try:
            assert calls() == [("mfma-check", tokens[0]), ("mfma-check", tokens[1])]
            devs = {d["ID"]: d for d in p.devices}
            assert devs[ids[0]]["health"] == "Healthy" and HEALTH_REASON_ATTR not in devs[ids[0]]["Attributes"]
            assert devs[ids[1]]["health"] == "Unhealthy"
            assert p.reasons[ids[1]].startswith("probe: mfma-check failed rc=1"), p.reasons
            assert "errors" in p.reasons[ids[1]]                      # the tail of the probe's stdout
            assert devs[ids[1]]["Attributes"][HEALTH_REASON_ATTR].startswith("probe_mfma-check")
            # sticky across health ticks until the operator resets it (the ticks are driven by hand)
            p._check_health()
            assert {d["ID"]: d["health"] for d in p.devices}[ids[1]] == "Unhealthy"
            request_reset(state, [ids[1]])
            p._apply_resets()
            p._check_health()
            devs = {d["ID"]: d for d in p.devices}
            assert devs[ids[1]]["health"] == "Healthy" and HEALTH_REASON_ATTR not in devs[ids[1]]["Attributes"]
        finally:
            await p.stop()
    run(go())


def test_hbm_and_mfma_run_both_hbm_first(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]

    async def go():
        p = await _start(fb, short_tmp, "hbm,mfma")
        try:
            got = calls()
            assert sorted(got) == sorted((n, t) for n in ("hbm-probe", "mfma-check") for t in tokens)
            for t in tokens:                                          # per GPU: the HBM probe before the matrix cores
                assert got.index(("hbm-probe", t)) < got.index(("mfma-check", t))
            assert got[0][0] == "hbm-probe"
            assert all(d["health"] == "Healthy" for d in p.devices)
        finally:
            await p.stop()
    run(go())


def test_mfma_is_not_run_on_a_gpu_whose_hbm_probe_failed(short_tmp, stubs):
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    ids = [device_id(g) for g in fb.gpus()]
    make("hbm-probe", tokens[0])

    async def go():
        p = await _start(fb, short_tmp, "mfma,hbm")                  # the order given does not matter
        try:
            assert calls() == [("hbm-probe", tokens[0]), ("hbm-probe", tokens[1]), ("mfma-check", tokens[1])]
            assert p.reasons[ids[0]].startswith("probe: hbm-probe failed rc=1")
            assert {d["ID"]: d["health"] for d in p.devices} == {ids[0]: "Unhealthy", ids[1]: "Healthy"}
        finally:
            await p.stop()
    run(go())


def test_hbm_alone_runs_only_the_hbm_probe(short_tmp, stubs):
    make, calls = stubs
    make()
    fb = FakeBackend(n=2)

    async def go():
        p = await _start(fb, short_tmp, "hbm")
        try:
            assert [n for n, _ in calls()] == ["hbm-probe", "hbm-probe"]
        finally:
            await p.stop()
    run(go())


def test_none_runs_no_probe(short_tmp, stubs):
    make, calls = stubs
    make()

    async def go():
        p = await _start(FakeBackend(n=2), short_tmp, "none")
        try:
            assert calls() == []
        finally:
            await p.stop()
    run(go())


@pytest.mark.parametrize("spec", ["foo", "hbm,foo", "", "none,hbm"])
def test_unknown_probe_name_is_refused_at_construction(short_tmp, spec):
    with pytest.raises(ValueError):
        amd.AMDGPUPlugin(FakeBackend(n=2), plugins_dir=str(short_tmp / "plugins"), health_probe=spec)


def test_cli_accepts_the_probe_lists():
    from amdkube.cmd.components import device_plugin_parser
    ap = device_plugin_parser()
    for spec in ("none", "hbm", "mfma", "hbm,mfma"):
        assert ap.parse_args(["--health-probe", spec]).health_probe == spec
        amd.parse_health_probe(spec)
    with pytest.raises(SystemExit):
        ap.parse_args(["--health-probe", "foo"])


def test_builtin_image_resolves_to_the_binary():
    from amdkube.runtime.images import builtin_images
    ent = builtin_images()["amdkube/mfma-check:latest"]["entrypoint"]
    assert os.path.basename(ent[0]) == "mfma-check" and os.path.dirname(ent[0]).endswith(os.path.join("_native", "bin"))
