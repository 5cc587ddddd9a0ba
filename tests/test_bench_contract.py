"""bench.py's driver contract on CPU: torchrun with 2 ranks over gloo, rank 0 drives the node
(fake 8xMI355X backend, busybox pods instead of the gfx950 vector-add), every rank brackets the
timed steps with barriers, the elapsed time is MAX-reduced and rank 0 prints one JSON line."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# the gloo rehearsals hide the node's GPUs from their ranks: with a GPU visible bench.py takes nccl,
# which refuses several ranks on one device
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def test_bench_two_ranks_gloo():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AMDKUBE_REQUIRE_NATIVE="0", **NO_GPU)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "fake", "--no-sched-perf", "--density-nodes", "0", "--image", "busybox",
           "--pod-arg=-c", "--pod-arg=true"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "pods/s"
    assert d["metric"].startswith("p50 GPU-pod startup latency") and d["higher_is_better"] is True
    assert d["gpu_pods"] == 4 and d["failed_pods"] == 0, d
    assert d["cpu_pods"] == 2 * round(22 * 2 / 8)
    assert d["value"] > 0 and abs(d["value"] - (d["gpu_pods"] + d["cpu_pods"]) / (d["ms_per_step"] * d["steps"] / 1000)) < 0.05 * d["value"]


def test_bench_eight_ranks_gloo_fake_8gpu_node():
    """The driver's N=8 launch rehearsed on CPU: torchrun --nproc-per-node 8 over gloo, a fake
    8×MI355X node, busybox GPU pods. One JSON line, n_gpus 8, every step's 8 GPU pods on 8
    distinct device IDs, and the timed region MAX-reduced over the 8 ranks."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AMDKUBE_REQUIRE_NATIVE="0", OMP_NUM_THREADS="1", **NO_GPU)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--backend", "fake", "--no-sched-perf", "--no-node-density", "--density-nodes", "0", "--image", "busybox",
           "--pod-arg=-c", "--pod-arg=true"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["steps"] == 2 and d["failed_pods"] == 0, d
    assert d["gpu_pods"] == 16 and d["cpu_pods"] == 2 * 22
    assert d["gpu_devices_per_step"] == [8, 8], d["gpu_devices_per_step"]
    assert len(d["gpu_devices_seen"]) == 8
    assert d["config"]["parallelism"] == "8 allocatable MI355X"


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """Without --full nothing but the timed steps is measured; --steps sets how many there are, and
    --dump-outputs writes the last step's pod outcomes as float32 arrays."""
    import numpy as np
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AMDKUBE_REQUIRE_NATIVE="0")
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "fake",
           "--image", "busybox", "--pod-arg=-c", "--pod-arg=true", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["gpu_pods"] == 3 * 2 and d["gpu_devices_per_step"] == [2, 2, 2] and d["failed_pods"] == 0, d
    assert d["ms_per_step"] > 0 and d["dtype"] == "fp32" and d["unit"] == "pods/s" and d["higher_is_better"] is True
    assert d["sched_perf"] is None and d["density"] is None and "node_density" not in d
    got = {p.name: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert sorted(got) == ["gpu_pod_devices_assigned.npy", "gpu_pod_exit_code.npy", "pod_is_gpu.npy", "pod_reached_goal.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    n_cpu = round(22 * 2 / 8)
    assert got["pod_is_gpu.npy"].tolist() == [1.0] * 2 + [0.0] * n_cpu
    assert got["pod_reached_goal.npy"].tolist() == [1.0] * (2 + n_cpu)
    assert got["gpu_pod_exit_code.npy"].tolist() == [0.0, 0.0] and got["gpu_pod_devices_assigned.npy"].tolist() == [1.0, 1.0]


def test_bench_node_density_fields_single_rank():
    """The density_test.go fields (batch of 10, 10-in-sequence with 50 background, kubelet and
    runtime CPU/RSS, API p99) are reported beside their limits."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", AMDKUBE_REQUIRE_NATIVE="0")
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0", "--backend", "fake", "--full",
           "--no-sched-perf", "--density-nodes", "0", "--image", "busybox", "--pod-arg=-c", "--pod-arg=true"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    nd = d["node_density"]
    assert "error" not in nd, nd
    for k in ("batch10_startup_ms", "seq10_bg50_startup_ms"):
        assert set(d[k]) == {"p50", "p90", "p99"} and 0 < d[k]["p50"] <= d[k]["p99"]
    for k in ("kubelet_cpu_cores_p50", "kubelet_cpu_cores_p95", "runtime_cpu_cores_p50", "runtime_rss_mib",
              "kubelet_rss_mib", "api_p99_ms", "batch10_batch_ms"):
        assert d[k] is not None and d[k] >= 0, k
    assert nd["limits"]["api_p99_ms"] == 1000 and nd["limits"]["kubelet_rss_mib"] == 100
    assert isinstance(nd["within_limits"], bool)
