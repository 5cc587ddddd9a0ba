"""Device-plugin side of the FP64 / INT8 matrix-core check: `mfma_check_dtype` / `--mfma-check-dtype`, run
against stub probe binaries that log their arguments, on the fake backend (CPU tier). Like the HBM march
it is no entry of the probe tables: it follows the `--health-probe` list, before `hbm-check`, or runs
alone with `none`."""
import pytest

from amdkube.deviceplugin import amd
from amdkube.smi import FakeBackend, device_id
from amdkube.smi.backend import visibility_token
from tests.conftest import run
from tests.probe_stubs import start as _start
from tests.test_hbm_check_plugin import stubs  # noqa: F401  (the fixture: stub probes with an hbm-check beside them)

HBM_ARGS, WIDE_ARGS = "--mib 512 --iters 2", "--dtype fp64,int8 --ms 200"


def _plugin_calls(short_tmp, stubs, probe, fail="", fail_gpu=None, **kw):  # noqa: F811
    """(calls, tokens, ids, plugin state) of one plugin start on two fake GPUs."""
    make, calls = stubs
    fb = FakeBackend(n=2)
    tokens = [visibility_token(g) for g in fb.gpus()]
    make(fail, tokens[fail_gpu] if fail_gpu is not None else "")

    async def go():
        p = await _start(fb, short_tmp, probe, **kw)
        try:
            p._check_health()                                         # a probe reason is sticky across health ticks
            return {d["ID"]: d["health"] for d in p.devices}, dict(p.reasons)
        finally:
            await p.stop()
    health, reasons = run(go())
    return calls(), tokens, [device_id(g) for g in fb.gpus()], health, reasons


def test_flag_off_means_no_extra_call(short_tmp, stubs):
    calls, tokens, _, _, _ = _plugin_calls(short_tmp, stubs, "hbm")
    assert calls == [("hbm-probe", t, HBM_ARGS) for t in tokens]


def test_flag_on_runs_one_check_per_gpu_after_the_list_and_before_hbm_check(short_tmp, stubs):
    calls, tokens, _, health, _ = _plugin_calls(short_tmp, stubs, "hbm", mfma_check_dtype="fp64,int8", hbm_check_mib=512)
    assert calls == [c for t in tokens for c in (("hbm-probe", t, HBM_ARGS), ("mfma-check", t, WIDE_ARGS),
                                                 ("hbm-check", t, "--mib 512"))]
    assert set(health.values()) == {"Healthy"}


def test_flag_on_runs_alone_with_none(short_tmp, stubs):
    calls, tokens, _, health, _ = _plugin_calls(short_tmp, stubs, "none", mfma_check_dtype="fp64,int8")
    assert calls == [("mfma-check", t, WIDE_ARGS) for t in tokens] and set(health.values()) == {"Healthy"}


def test_a_failing_run_sets_the_sticky_reason_and_ends_the_chain(short_tmp, stubs):
    calls, tokens, ids, health, reasons = _plugin_calls(short_tmp, stubs, "hbm", fail="--dtype fp64", fail_gpu=1,
                                                        mfma_check_dtype="fp64,int8", hbm_check_mib=512)
    assert [c[0] for c in calls if c[1] == tokens[1]] == ["hbm-probe", "mfma-check"]
    assert [c[0] for c in calls if c[1] == tokens[0]] == ["hbm-probe", "mfma-check", "hbm-check"]
    assert health == {ids[0]: "Healthy", ids[1]: "Unhealthy"}
    assert reasons[ids[1]].startswith("probe: mfma-check failed rc=1"), reasons


def test_an_earlier_probe_failure_skips_it(short_tmp, stubs):
    calls, tokens, ids, health, _ = _plugin_calls(short_tmp, stubs, "hbm", fail="hbm-probe", fail_gpu=0,
                                                  mfma_check_dtype="fp64,int8")
    assert calls == [("hbm-probe", tokens[0], HBM_ARGS), ("hbm-probe", tokens[1], HBM_ARGS),
                     ("mfma-check", tokens[1], WIDE_ARGS)]
    assert health == {ids[0]: "Unhealthy", ids[1]: "Healthy"}


def test_the_parser_and_the_constructor_refuse_an_unknown_name():
    from amdkube.cmd.components import device_plugin_parser
    ap = device_plugin_parser()
    assert ap.parse_args([]).mfma_check_dtype == ""
    assert ap.parse_args(["--mfma-check-dtype", "fp64,int8"]).mfma_check_dtype == "fp64,int8"
    assert ap.parse_args(["--mfma-check-dtype", "int8", "--health-probe", "none"]).mfma_check_dtype == "int8"
    for bad in ("fp16", "fp64,fp6", "fp64,", "wide"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--mfma-check-dtype", bad])
        with pytest.raises(ValueError):
            amd.AMDGPUPlugin(FakeBackend(n=1), mfma_check_dtype=bad)
