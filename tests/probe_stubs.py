"""Stub probe binaries for the device-plugin health-probe tests (test_mfma_probe_plugin.py,
test_mfma_lp_probe_plugin.py, test_cu_probe_plugin.py): shell scripts in place of hbm-probe,
mfma-check and cu-check that log how they were run, one of which can be made to fail."""
import stat

from amdkube.deviceplugin import amd

# logs `<name> <token> <arguments>`; the run whose `<name> <arguments>` contains `fail` exits 1 on the GPU `fail_token`
STUB = """#!/bin/sh
echo "{name} $ROCR_VISIBLE_DEVICES $@" >> "{log}"
echo '{{"errors":3}}'
case "{name} $@" in *"{fail}"*) if [ -n "{fail}" ] && [ "$ROCR_VISIBLE_DEVICES" = "{fail_token}" ]; then exit 1; fi;; esac
exit 0
"""


def make_stubs(short_tmp, monkeypatch, fields=3):
    """The body of a `stubs` fixture: BIN_DIR → a directory of stub probes. Returns (make, calls):
    make(fail, fail_token) writes them so that the run matching `fail` (a binary's name, or any part
    of `<name> <arguments>`) exits 1 for one GPU's token; calls() is the log so far, as
    [(binary, token, arguments)] cut to its first `fields` fields."""
    bindir = short_tmp / "bin"
    bindir.mkdir()
    log = short_tmp / "probe.log"
    monkeypatch.setattr(amd, "BIN_DIR", str(bindir))

    def make(fail="", fail_token=""):
        for name in ("hbm-probe", "mfma-check", "cu-check"):
            p = bindir / name
            p.write_text(STUB.format(name=name, log=log, fail=fail, fail_token=fail_token))
            p.chmod(p.stat().st_mode | stat.S_IXUSR)

    def calls():
        return [tuple(line.split(" ", 2)[:fields]) for line in log.read_text().splitlines()] if log.exists() else []
    return make, calls


def start(fb, tmp, probe, **kw):
    async def go():
        p = amd.AMDGPUPlugin(fb, plugins_dir=str(tmp / "plugins"), health_interval=3600.0, health_probe=probe, **kw)
        await p.start()
        return p
    return go()
