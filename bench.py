"""amdkube headline benchmark: pod density throughput + p50 GPU-pod startup latency on one
MI355X node with N allocatable GPUs (BASELINE.json metric; SURVEY §6 mapping).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--mode density|churn] [--dump-outputs DIR] [--full]
  torchrun --nproc-per-node N bench.py --gpus N ...   (one rank per GPU; rank 0 drives)

Rank 0 launches the node (apiserver, scheduler, rocshim, AMD device plugin on amd-smi,
kubelet) in a child process BEFORE any GPU initialisation in this process, then every rank
brackets exactly K steps with barrier + torch.cuda.synchronize().

density (default) — the reference's headline test, test/e2e/scalability/density.go (30 pods
per node; saturation throughput ≥ 8 pods/s, startup p50/p90/p99 ≤ 5 s), run on the real
MI355X node: one step creates N GPU pods (`amd.com/gpu: 1` each through ResourceV2 →
device-granular binding, running the real gfx950 vector-add to completion on exactly its
assigned GPU) plus the density share of pause pods (22 per 8 GPUs, i.e. 30 pods at N=8);
the step ends when every pause pod is Running and every GPU pod has Succeeded.
value = all pods per second over the job; gpu_pods_per_s, GPU-pod and all-pod startup
percentiles are reported beside it. churn — GPU pods only, P per GPU per step (the per-GPU
process-lifetime bound; docs/PERFORMANCE.md).

Baselines: density saturation ≥ 8 pods/s (vs_baseline = value / 8),
pod startup p50/p90/p99 ≤ 5 s, scheduler throughput ≥ 30 pods/s (goal 100).

A plain run sets up the node, warms up, times the K steps, writes the last step's pod outcomes
if --dump-outputs is given (per pod: GPU pod or not, goal reached; per GPU pod: exit code, GPUs
assigned) and prints the result line. Extra fields, only with --full and
all measured after the timed region: the node-density tests of test/e2e_node/density_test.go
(batch of 10, 10 in sequence beside 50 background pods) with the kubelet's and runtime's CPU
cores p50/p95 and RSS and the API call p99, each beside its reference limit
(podbench.DENSITY_LIMITS); scheduler_perf (100 nodes / 3000 pods); the density test on 100
hollow 8×MI355X nodes (amdkube/benchmark/density.py).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
METRIC = "p50 GPU-pod startup latency + scheduling throughput (pods/s) at 1/2/4/8 MI355X"
BASELINE_PODS_PER_S = 8.0      # test/e2e/scalability/density.go:55-56 MinPodsPerSecondThroughput
SLO_STARTUP_MS = 5000.0        # test/e2e/framework/metrics_util.go:46


def dump_outputs(path, last_step):
    """What the timed path handed back for its last step, one float32 array per name. The step's
    inputs are fixed by the arguments (N GPU pods adding the same 50,000 seeded fp32 elements,
    the density share of pause pods), so two builds run with the same arguments compare array
    for array; timings are left out."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for name, values in last_step.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(values, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pods-per-gpu", type=int, default=4, help="churn mode only")
    ap.add_argument("--mode", default="density", choices=("density", "churn"),
                    help="density: the reference density.go mix on the real node (default); churn: GPU pods only")
    ap.add_argument("--backend", default="auto", help="amdsmi|sysfs|fake|auto")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the node-density tests, scheduler_perf and the hollow-node "
                         "density run (each can be dropped with the three options below)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step's pods came to as DIR/<name>.npy (float32)")
    ap.add_argument("--no-sched-perf", action="store_true", help="with --full: skip scheduler_perf")
    ap.add_argument("--no-node-density", action="store_true",
                    help="with --full: skip the density_test.go batch/sequence tests with resource sampling")
    ap.add_argument("--density-nodes", type=int, default=100, help="with --full: hollow-node density run (0 = skip)")
    ap.add_argument("--image", default="rocm/vector-add", help="GPU pod image (CPU rehearsals: busybox)")
    ap.add_argument("--pod-arg", action="append", default=[], help="GPU pod container argument (repeatable)")
    ap.add_argument("--isolation", default=None, help="rocshim device isolation (default: auto on real GPUs)")
    a = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n = a.gpus or world

    worker = None
    if rank == 0:
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env["AMDKUBE_REQUIRE_NATIVE"] = "1"
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR", "MASTER_PORT",
                  "TORCHELASTIC_RUN_ID"):
            env.pop(k, None)
        worker = subprocess.Popen([sys.executable, "-m", "amdkube.benchmark.podbench", "--gpus", str(n),
                                   "--pods-per-gpu", str(a.pods_per_gpu), "--backend", a.backend, "--mode", a.mode,
                                   "--image", a.image, *(["--isolation", a.isolation] if a.isolation else []),
                                   "--", *a.pod_arg],
                                  cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        ready = json.loads(worker.stdout.readline() or "{}")
        if not ready.get("ready"):
            worker.kill()
            raise SystemExit("cluster worker failed to start")
        print(f"[bench] node ready: {len(ready['gpus'])} GPU(s) via {ready['backend']}, isolation={ready.get('isolation')}",
              file=sys.stderr, flush=True)

    import torch
    import torch.distributed as dist
    cuda = torch.cuda.is_available()
    if cuda:
        torch.cuda.set_device(local_rank % max(1, torch.cuda.device_count()))
    if world > 1:
        dist.init_process_group("nccl" if cuda else "gloo")

    def barrier():
        if world > 1:
            if cuda:
                dist.barrier(device_ids=[torch.cuda.current_device()])
            else:
                dist.barrier()

    def sync():
        if cuda:
            torch.cuda.synchronize()

    def drive(steps):
        worker.stdin.write(json.dumps({"cmd": "run", "steps": steps}) + "\n")
        worker.stdin.flush()
        return json.loads(worker.stdout.readline())

    if rank == 0 and a.warmup > 0:
        drive(a.warmup)
    barrier()
    sync()
    t0 = time.perf_counter()
    res = drive(a.steps) if rank == 0 else None
    barrier()
    sync()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device="cuda" if cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    if rank == 0:
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, res["last_step"])
        node_density = None
        if a.full and not a.no_node_density:
            worker.stdin.write(json.dumps({"cmd": "node_density"}) + "\n")
            worker.stdin.flush()
            node_density = json.loads(worker.stdout.readline())
        sched = None
        if a.full and not a.no_sched_perf:
            worker.stdin.write(json.dumps({"cmd": "schedperf", "nodes": 100, "pods": 3000}) + "\n")
            worker.stdin.flush()
            sched = json.loads(worker.stdout.readline())
        density = None
        if a.full and a.density_nodes:
            # the reference's headline density test (30 pods/node saturation) on hollow MI355X nodes;
            # a child process so its control plane does not share this rank's core (not timed)
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
            try:
                r = subprocess.run([sys.executable, "-m", "amdkube.benchmark.density", "--nodes", str(a.density_nodes),
                                    "--node-procs", "6"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                density = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stderr[-500:]}
            except Exception as e:
                density = {"error": repr(e)}
        worker.stdin.write(json.dumps({"cmd": "quit"}) + "\n")
        worker.stdin.flush()
        try:
            worker.wait(60)
        except subprocess.TimeoutExpired:
            worker.kill()
        pods = res["pods"]
        value = pods / el
        if a.mode == "density":
            data = (f"synthetic: per step {n} rocm/vector-add GPU pod(s) (one per allocatable MI355X, 50,000 fp32 elements, run to "
                    f"completion on the assigned GPU) + {res['cpu_pods'] // a.steps} pause pods, the reference density.go mix of "
                    "30 pods/node at 8 GPUs scaled to N")
            model = "density.go on one real MI355X node: GPU pods (amd.com/gpu=1, ResourceV2 → device binding) + pause pods"
            gbatch = res["pods"] // a.steps
        else:
            data = "synthetic: rocm/vector-add GPU pods (50,000 fp32 elements each, cuda-vector-add equivalent)"
            model = "GPU-pod churn: 1 node, amd.com/gpu=1 pods, ResourceV2 → device-granular binding"
            gbatch = n * a.pods_per_gpu
        out = {"metric": METRIC, "value": round(value, 3), "unit": "pods/s", "n_gpus": n, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(el * 1000 / a.steps, 2), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": round(value / BASELINE_PODS_PER_S, 3), "dtype": "fp32", "data": data,
               "config": {"model": model, "global_batch": gbatch, "seq_len": None, "parallelism": f"{n} allocatable MI355X",
                          "mode": a.mode},
               "gpu_pods_per_s": round(res["gpu_pods"] / el, 3), "gpu_pods": res["gpu_pods"], "cpu_pods": res["cpu_pods"],
               "p50_startup_ms": res["p50_startup_ms"], "p90_startup_ms": res["p90_startup_ms"],
               "p99_startup_ms": res["p99_startup_ms"], "startup_slo_ms": SLO_STARTUP_MS,
               "p50_startup_all_pods_ms": res["p50_startup_all_pods_ms"], "p99_startup_all_pods_ms": res["p99_startup_all_pods_ms"],
               "p50_node_startup_ms": res["p50_node_startup_ms"], "p50_schedule_ms": res["p50_schedule_ms"],
               "p50_pod_runtime_ms": res["p50_pod_runtime_ms"], "failed_pods": res["failed"],
               "node_cpu_s": res.get("node_cpu_s"), "isolation": ready.get("isolation"),
               "gpu_devices_per_step": res.get("gpu_devices_per_step"), "gpu_devices_seen": res.get("gpu_devices_seen"),
               "sched_perf": sched, "density": density}
        if node_density is not None:
            # the reference node-density thresholds (test/e2e_node/density_test.go, metrics_util.go),
            # each value beside its limit in node_density["limits"]
            for k in ("kubelet_cpu_cores_p50", "kubelet_cpu_cores_p95", "runtime_cpu_cores_p50", "runtime_cpu_cores_p95",
                      "kubelet_rss_mib", "runtime_rss_mib", "batch10_startup_ms", "batch10_batch_ms",
                      "seq10_bg50_startup_ms", "api_p99_ms"):
                out[k] = node_density.get(k)
            out["node_density"] = node_density
        if res["failed"]:
            out["failures"] = res["failures"]
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
