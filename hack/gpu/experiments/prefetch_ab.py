"""Does prefetching the files hsa_init reads, during its /dev/kfd wait, shorten a GPU pod on MI355X?

  prefetch_ab.py process OUT.json [--parent BIN]   hsa-vector-add processes with AMDKUBE_VADD_TRACE=1
  prefetch_ab.py bench OUTDIR [--parent BIN]       bench.py --gpus 1 --steps 20 --warmup 5

process: 15 rounds back to back, alternating the arms (prefetch on, --no-prefetch and, with --parent,
the parent commit's binary) so that every run has a predecessor that exited the same way; then 8
rounds with a 1 s idle gap before every run (no predecessor's KFD release work to wait for).
Records each run's wall time, phase lines and I/O groups; prints median and min–max per arm.

bench: three runs of each arm, alternating, then (with --parent) one run with the parent commit's
binary in place of hsa-vector-add, and a --dump-outputs comparison of a prefetch run with it.

Every child has its own time limit and the driver stops at the first one that fails.
"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin", "hsa-vector-add")

PHASE = re.compile(r"^\[trace\] (?!io |prefetch )(.+?)\s+([\d.]+) ms$", re.M)
IO = re.compile(r"^\[trace\] io (\S+)\s+(.*)$", re.M)
PREFETCH = re.compile(r"^\[trace\] prefetch (\S+) (.*)$", re.M)


def kv(text):
    return {k: float(v) for k, v in (p.split("=") for p in text.split())}


def run_once(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=dict(os.environ, AMDKUBE_VADD_TRACE="1"), capture_output=True, text=True, timeout=60)
    wall = (time.perf_counter() - t0) * 1000
    if r.returncode != 0 or "Test PASSED" not in r.stdout:
        raise SystemExit(f"{cmd} failed ({r.returncode}):\n{r.stdout[-500:]}\n{r.stderr[-1500:]}")
    out = {"wall_ms": round(wall, 2), "phases": {m.group(1): float(m.group(2)) for m in PHASE.finditer(r.stderr)},
           "io": {m.group(1): kv(m.group(2)) for m in IO.finditer(r.stderr)}}
    m = PREFETCH.search(r.stderr)
    if m:
        out["prefetch"] = dict(kv(m.group(2)), state=m.group(1))
    return out


def spread(values):
    values = [v for v in values if v is not None]
    if not values:
        return None
    return {"median": round(statistics.median(values), 2), "min": round(min(values), 2), "max": round(max(values), 2),
            "n": len(values)}


def summarise(runs):
    ph = lambda name: [r["phases"].get(name) for r in runs]  # noqa: E731
    io = lambda g, k: [r["io"].get(g, {}).get(k) for r in runs]  # noqa: E731
    s = {"wall_ms": spread([r["wall_ms"] for r in runs]), "hsa_init": spread(ph("hsa_init")),
         "init:pre-open": spread(ph("init:pre-open")), "init:kfd-wait": spread(ph("init:kfd-wait")),
         "init:post-wait": spread(ph("init:post-wait")), "shut down": spread(ph("shut down")),
         # from the memory pools to the created queue
         "pools..queue": spread([sum(r["phases"].get(p, 0.0) for p in ("code object", "alloc + fill", "queue"))
                                 for r in runs])}
    for g in ("kfd-topology", "/proc", "/sys/devices/system", "drm+pci", "/dev", "other"):
        s["io " + g] = {k: spread(io(g, k)) for k in ("fopen", "fopen_ms", "open", "open_ms", "opendir", "opendir_ms")}
    if any("prefetch" in r for r in runs):
        s["prefetch"] = {k: spread([r.get("prefetch", {}).get(k) for r in runs]) for k in ("files", "bytes", "helper_ms", "hits", "misses", "distinct")}
    return s


def process(a):
    arms = [("prefetch", [BIN, "-n", "50000"]), ("no-prefetch", [BIN, "-n", "50000", "--no-prefetch"])]
    if a.parent:
        arms.append(("parent", [a.parent, "-n", "50000"]))
    res = {"runs": {}}
    run_once(arms[-1][1])                                  # give the first timed run a predecessor too
    for cadence, rounds in (("back_to_back", 15), ("idle", 8)):
        for rnd in range(rounds):
            for name, cmd in arms:
                if cadence == "idle":
                    time.sleep(1.0)
                r = run_once(cmd)
                res["runs"].setdefault(f"{name}/{cadence}", []).append(r)
                print(name, cadence, rnd, r["wall_ms"], r["phases"].get("hsa_init"), r["phases"].get("init:post-wait"), flush=True)
    res["summary"] = {k: summarise(v) for k, v in res["runs"].items()}
    print(json.dumps(res["summary"], indent=1), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


def bench_once(extra, dump=None):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", *extra]
    if dump:
        cmd += ["--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        raise SystemExit(f"bench failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def find(d, key):
    if isinstance(d, dict):
        if key in d:
            return d[key]
        for v in d.values():
            x = find(v, key)
            if x is not None:
                return x
    return None


def bench(a):
    import numpy as np
    os.makedirs(a.out, exist_ok=True)
    rows = []

    def one(arm, extra, dump=None):
        j = bench_once(extra, dump)
        row = {"arm": arm, "value": j.get("value"), "ms_per_step": find(j, "ms_per_step"),
               "p50_pod_runtime_ms": find(j, "p50_pod_runtime_ms"), "failed_pods": find(j, "failed_pods")}
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(os.path.join(a.out, f"bench_{len(rows)}_{arm}.json"), "w") as f:
            json.dump(j, f, indent=1)
        if row["failed_pods"] != 0:
            raise SystemExit(f"failed pods in {arm}")

    for i in range(3):
        one("prefetch", [], os.path.join(a.out, "dump_prefetch") if i == 0 else None)
        one("no-prefetch", ["--pod-arg=--no-prefetch"])
    if a.parent:
        shutil.copy2(BIN, BIN + ".new")
        try:
            shutil.copy2(a.parent, BIN)
            one("parent", [], os.path.join(a.out, "dump_parent"))
        finally:
            os.replace(BIN + ".new", BIN)
        same = {}
        for name in sorted(os.listdir(os.path.join(a.out, "dump_parent"))):
            x = np.load(os.path.join(a.out, "dump_parent", name))
            y = np.load(os.path.join(a.out, "dump_prefetch", name))
            same[name] = bool(x.shape == y.shape and np.array_equal(x, y))
        print("dump-outputs equal:", json.dumps(same), flush=True)
        rows.append({"arm": "dump-outputs prefetch == parent", **same})
    on = [r["ms_per_step"] for r in rows if r["arm"] == "prefetch"]
    off = [r["ms_per_step"] for r in rows if r["arm"] == "no-prefetch"]
    verdict = {"prefetch": spread(on), "no-prefetch": spread(off),
               "mean_difference_ms": round(statistics.mean(off) - statistics.mean(on), 2),
               "larger_spread_ms": round(max(max(on) - min(on), max(off) - min(off)), 2),
               "every_prefetch_run_below_every_no_prefetch_run": max(on) < min(off)}
    verdict["gain"] = verdict["every_prefetch_run_below_every_no_prefetch_run"] and \
        verdict["mean_difference_ms"] > verdict["larger_spread_ms"]
    print(json.dumps(verdict, indent=1), flush=True)
    with open(os.path.join(a.out, "bench_ab.json"), "w") as f:
        json.dump({"runs": rows, "verdict": verdict}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("process", "bench"))
    ap.add_argument("out")
    ap.add_argument("--parent", default=None, help="hsa-vector-add built from the parent commit")
    a = ap.parse_args()
    process(a) if a.what == "process" else bench(a)


if __name__ == "__main__":
    main()
