"""GPU tier: the checked matrix-core workload (kernels/mfma_check.h) through every layer: the
mfma-check and gpu-burn --verify binaries, the device plugin's mfma probe, and the in-process ops.

The tests that start child processes come first, as in test_gpu.py; each child is a fresh process.
torch is imported inside the tests, as in test_gpu.py: collecting this file must not load the ROCm
libraries into the process before the amd-smi tests of the tier have run.

Numerics: on integer data in [-8, 8] every product and partial sum is an exact fp32 integer, so the
LDS-staged MFMA GEMM must equal the fp32 matmul bit for bit; on random data the bound is
|c - ref| <= K * 2^-23 * (|A| @ |B|) against a float64 product of the bf16-rounded inputs (a bf16
product is exact in fp32, any-order fp32 summation of K terms is within K * 2^-24 * sum|a b|, and
the bound carries a factor 2 over that).
"""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

from amdkube.localcluster import LocalCluster  # noqa: E402
from tests.conftest import run  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")


def _bin(name, *args):
    r = subprocess.run([os.path.join(BIN, name), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, json.loads(r.stdout), r


# ---------------------------------------------------------------- binaries and the plugin
def test_mfma_check_binary_passes_on_a_healthy_gpu():
    rc, d, r = _bin("mfma-check", "--rounds", "2")
    assert rc == 0 and d["errors"] == 0 and d["first_errors"] == [], (r.stdout, r.stderr)
    assert d["rounds"] == 2 and d["k"] == 128 and d["blocks"] > 0 and d["arch"].startswith("gfx950")
    assert d["uuid"].startswith("GPU-") and d["bf16_tflops"] > 0


def test_mfma_check_binary_reports_selftest_flips():
    rc, d, r = _bin("mfma-check", "--rounds", "2", "--selftest-flips", "5")
    assert rc == 1 and d["errors"] == 5 and len(d["first_errors"]) == 5, (r.stdout, r.stderr)


def test_gpu_burn_verify():
    rc, d, r = _bin("gpu-burn", "--ms", "100", "--verify")
    assert rc == 0 and d["verified"] is True and d["errors"] == 0 and d["bf16_tflops"] > 0, (r.stdout, r.stderr)


def test_plugin_hbm_and_mfma_probes_mark_healthy():
    async def go():
        async with LocalCluster(gpus="amdsmi", n_gpus=1, with_controllers=False, health_probe="hbm,mfma") as lc:
            node = await lc.wait_gpus(1, 120)
            devs = node["status"]["extendedResources"]["amd.com/gpu"]["resources"]
            assert devs and all(d["health"] == "Healthy" for d in devs.values()), lc.plugin.reasons
    run(go(), 300)


# ---------------------------------------------------------------- mfma_gemm
def _ints(shape, gen):
    import torch
    return torch.randint(-8, 9, shape, generator=gen).float()


@pytest.mark.parametrize("m,n,k", [(64, 64, 16), (64, 64, 48), (128, 64, 80), (64, 192, 272)])
def test_mfma_gemm_is_exact_on_integer_data(m, n, k):
    import torch
    from amdkube.ops import hip
    g = torch.Generator().manual_seed(1000 * m + 10 * n + k)
    a, b = _ints((m, k), g), _ints((k, n), g)
    c = hip.mfma_gemm(a, b)
    assert c.dtype == torch.float32 and tuple(c.shape) == (m, n)
    assert torch.equal(c, a @ b)


def test_mfma_gemm_one_hot_a_picks_exact_rows_of_an_asymmetric_b():
    import torch
    from amdkube.ops import hip
    m, n, k = 128, 192, 80
    rows = (torch.arange(m) * 37 + 11) % k                            # which row of B each row of C must be
    a = torch.zeros(m, k)
    a[torch.arange(m), rows] = 1.0
    b = (torch.arange(k).float()[:, None] * n + torch.arange(n).float()[None, :]) / 64      # B[i][j] = (i N + j) / 64
    b = b.to(torch.bfloat16).float()                                  # as the matrix core sees it
    assert not torch.equal(b[:k, :k], b[:k, :k].T) and b.unique(dim=0).shape[0] == k         # asymmetric, rows distinct
    c = hip.mfma_gemm(a, b)
    assert torch.equal(c, b[rows])


def test_mfma_gemm_random_data_within_the_fp32_summation_bound():
    import torch
    from amdkube.ops import hip
    m, n, k = 128, 128, 256
    g = torch.Generator().manual_seed(7)
    a = torch.randn(m, k, generator=g).to(torch.bfloat16)
    b = torch.randn(k, n, generator=g).to(torch.bfloat16)
    ref = a.double() @ b.double()
    bound = k * 2.0 ** -23 * (a.double().abs() @ b.double().abs())
    cpu = (a.float() @ b.float()).double()                            # torch's own fp32 matmul stays within it
    assert bool(((cpu - ref).abs() <= bound).all())
    c = hip.mfma_gemm(a, b).double()
    err = (c - ref).abs()
    print("mfma_gemm max |err| / bound:", float((err / bound).max()))
    assert bool((err <= bound).all())


def test_mfma_gemm_refuses_bad_shapes():
    import torch
    from amdkube.ops import hip
    with pytest.raises(ValueError):
        hip.mfma_gemm(torch.zeros(32, 16), torch.zeros(16, 64))       # M = 32
    with pytest.raises(ValueError):
        hip.mfma_gemm(torch.zeros(64, 24), torch.zeros(24, 64))       # K = 24
    with pytest.raises(ValueError):
        hip.mfma_gemm(torch.zeros(64, 32), torch.zeros(16, 64))       # inner dimensions differ


# ---------------------------------------------------------------- mfma_check
@pytest.fixture(scope="module")
def blocks():
    from amdkube.ops import hip
    return 4 * hip.device_info()["cu_count"]


@pytest.fixture(scope="module")
def tiles(blocks):
    from amdkube.ops import hip
    return {(blk, seed): hip.mfma_check_tile(blk, seed=seed) for blk in (0, blocks - 1) for seed in (0x5EED, 12345)}


def test_mfma_check_tile_operands_and_product(tiles):
    import torch
    for (blk, seed), (a, b, c) in tiles.items():
        assert tuple(a.shape) == (64, 128) and tuple(b.shape) == (128, 64) and tuple(c.shape) == (64, 64)
        for x in (a, b):
            assert torch.equal(x, x.round()) and float(x.min()) >= -8 and float(x.max()) <= 8
            assert x.unique().numel() == 17                           # all of [-8, 8] over 8192 hashed draws
        assert torch.equal(c, a @ b), (blk, seed)


def test_mfma_check_tile_inputs_differ_by_seed_and_block(tiles, blocks):
    import torch
    for blk in (0, blocks - 1):
        assert not torch.equal(tiles[(blk, 0x5EED)][0], tiles[(blk, 12345)][0])
        assert not torch.equal(tiles[(blk, 0x5EED)][1], tiles[(blk, 12345)][1])
    for seed in (0x5EED, 12345):
        assert not torch.equal(tiles[(0, seed)][0], tiles[(blocks - 1, seed)][0])
        assert not torch.equal(tiles[(0, seed)][1], tiles[(blocks - 1, seed)][1])
    assert not torch.equal(tiles[(0, 0x5EED)][0][:, :64], tiles[(0, 0x5EED)][1][:64, :])     # A is not B


def test_mfma_check_tile_refuses_a_block_outside_the_grid(blocks):
    from amdkube.ops import hip
    with pytest.raises(ValueError):
        hip.mfma_check_tile(blocks)


def test_mfma_check_clean_run(blocks):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2)
    assert r["ok"] is True and r["errors"] == 0 and r["first_errors"] == []
    assert r["blocks"] == blocks and r["rounds"] == 2 and r["k"] == 128
    assert r["bf16_tflops"] > 0 and r["ms"] > 0


def test_mfma_check_selftest_flips_are_all_reported(blocks):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, selftest_flips=37)
    assert r["errors"] == 37 and r["ok"] is False
    recs = r["first_errors"]
    assert len(recs) == 16
    for e in recs:
        assert 0 <= e["block"] < blocks and 0 <= e["row"] < 64 and 0 <= e["col"] < 64 and e["round"] in (0, 1), e
        assert e["got"] != e["want"] and e["got"] ^ e["want"] == 1, e    # the low mantissa bit of the compared copy
    assert {e["round"] for e in recs} == {0, 1}
    assert len({(e["block"], e["row"], e["col"], e["round"]) for e in recs}) == 16


def test_mfma_check_single_flip_single_round():
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=1, selftest_flips=1)
    assert r["errors"] == 1 and r["ok"] is False and len(r["first_errors"]) == 1
    assert r["first_errors"][0]["round"] == 0
