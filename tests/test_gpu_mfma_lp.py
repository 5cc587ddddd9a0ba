"""GPU tier: the low-precision matrix-core check (kernels/mfma_check_lp.h: the FP8 MFMA and the
block-scaled e4m3 / e2m1 forms) through every layer: mfma-check --dtype, the device plugin's mfma-lp
probe, and the in-process ops.

The tests that start child processes come first, as in test_gpu_mfma_check.py, and torch is imported
inside the tests for the same reason as there.

Numerics: every value of these formats times a power-of-two block scale is a small multiple of a
power of two, so on the data of the exact tests every product and partial sum is an fp32 number and
the GEMM must equal the float64 product of the decoded operands bit for bit. The one-hot tests pin
the operand and scale lane maps: a lane that fed another k, another row's scale or another nibble
would pick another row of B or scale it differently. On random data the bound is
|c - ref| <= K * 2^-23 * (|A| @ |B|) against a float64 product of the dequantised inputs: a product
of two such values is exact in fp32, any-order fp32 summation of K terms is within
K * 2^-24 * sum|a b|, and the bound carries a factor 2 over that, as in the bf16 test.
"""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

from amdkube.localcluster import LocalCluster  # noqa: E402
from tests.conftest import run  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
DTYPES = ("fp8", "mxfp8", "mxfp4")
K_OF = {"fp8": 256, "mxfp8": 256, "mxfp4": 512}


def _check(*args):
    r = subprocess.run([os.path.join(BIN, "mfma-check"), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


# ---------------------------------------------------------------- the binary and the plugin
def test_binary_checks_every_low_precision_dtype():
    rc, lines, r = _check("--dtype", "fp8,mxfp8,mxfp4", "--rounds", "2")
    assert rc == 0 and [d["dtype"] for d in lines] == list(DTYPES), (r.stdout, r.stderr)
    for d in lines:
        assert d["errors"] == 0 and d["first_errors"] == [] and d["rounds"] == 2 and d["k"] == K_OF[d["dtype"]], d
        assert d["tflops"] > 0 and d["blocks"] > 0 and d["arch"].startswith("gfx950") and "bf16_tflops" not in d, d


def test_binary_reports_selftest_flips_on_mxfp4():
    rc, lines, r = _check("--dtype", "mxfp4", "--rounds", "2", "--selftest-flips", "5")
    assert rc == 1 and len(lines) == 1, (r.stdout, r.stderr)
    assert lines[0]["dtype"] == "mxfp4" and lines[0]["errors"] == 5 and len(lines[0]["first_errors"]) == 5


def test_binary_stops_after_the_first_failing_dtype():
    rc, lines, r = _check("--dtype", "fp8,mxfp4", "--selftest-flips", "3", "--rounds", "1")
    assert rc == 1 and [d["dtype"] for d in lines] == ["fp8"] and lines[0]["errors"] == 3, (r.stdout, r.stderr)


def test_binary_without_dtype_prints_the_bf16_line_as_before():
    rc, lines, r = _check("--rounds", "2")
    assert rc == 0 and len(lines) == 1, (r.stdout, r.stderr)
    assert "dtype" not in lines[0] and "tflops" not in lines[0] and lines[0]["bf16_tflops"] > 0 and lines[0]["k"] == 128


def test_binary_bf16_in_a_dtype_list_and_an_unknown_dtype():
    rc, lines, r = _check("--dtype", "bf16,fp8", "--rounds", "1")
    assert rc == 0 and [d["dtype"] for d in lines] == ["bf16", "fp8"], (r.stdout, r.stderr)
    assert lines[0]["bf16_tflops"] > 0 and lines[0]["tflops"] > 0 and lines[0]["k"] == 128
    r = subprocess.run([os.path.join(BIN, "mfma-check"), "--dtype", "fp8,fp6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "" and "fp6" in r.stderr


def test_plugin_hbm_mfma_and_mfma_lp_probes_mark_healthy():
    async def go():
        async with LocalCluster(gpus="amdsmi", n_gpus=1, with_controllers=False, health_probe="hbm,mfma,mfma-lp") as lc:
            node = await lc.wait_gpus(1, 120)
            devs = node["status"]["extendedResources"]["amd.com/gpu"]["resources"]
            assert devs and all(d["health"] == "Healthy" for d in devs.values()), lc.plugin.reasons
    run(go(), 300)


# ---------------------------------------------------------------- one-hot: the operand and scale lane maps
def _asymmetric_codes(k, n, dtype):
    """K x N codes whose decoded rows are distinct and whose square part is not symmetric."""
    import numpy as np
    i, j = np.arange(k)[:, None], np.arange(n)[None, :]
    if dtype == "mxfp4":
        return (((i * 7919 + j * 104729 + i * j * 31) >> 3) % 16).astype(np.uint8)
    c = ((i * 131 + j * 17 + 5) % 256).astype(np.uint8)
    c[(c & 0x7F) == 0x7F] = 0x3C                                      # no NaN codes
    return c


def test_fp8_one_hot_a_picks_exact_rows_of_an_asymmetric_b():
    import numpy as np
    import torch
    from amdkube.ops import hip, lowp
    m, n, k = 128, 192, 80
    rows = (np.arange(m) * 37 + 11) % k
    a = np.zeros((m, k), np.float32)
    a[np.arange(m), rows] = 1.0
    b = lowp.decode_e4m3(_asymmetric_codes(k, n, "fp8"))
    assert not np.array_equal(b[:k, :k], b[:k, :k].T) and np.unique(b, axis=0).shape[0] == k
    c = hip.mfma_gemm_fp8(a, b)
    assert c.dtype == torch.float32 and tuple(c.shape) == (m, n)
    assert np.array_equal(c.numpy(), b[rows])


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_mx_one_hot_a_picks_exact_scaled_rows_of_an_asymmetric_b(fmt):
    import numpy as np
    from amdkube.ops import hip, lowp
    m, n, k = 128, 192, 192
    rows = (np.arange(m) * 37 + 11) % k
    one = int((lowp.encode_e4m3 if fmt == "fp8" else lowp.encode_e2m1)([1.0])[0])
    a = np.zeros((m, k), np.uint8)
    a[np.arange(m), rows] = one
    # no scale is 1, A's and B's differ, and neighbouring rows, columns and blocks differ
    a_exp = np.array([1, 2, -1])[(np.arange(m)[:, None] + np.arange(k // 32)[None, :]) % 3]
    b_exp = np.array([-2, 3, -1])[(2 * np.arange(k // 32)[:, None] + np.arange(n)[None, :]) % 3]
    b = _asymmetric_codes(k, n, "mx" + fmt)
    bdec = lowp.mx_dequantize(b, lowp.e8m0(b_exp), fmt, axis=0)
    assert not np.array_equal(bdec[:k, :k], bdec[:k, :k].T) and np.unique(bdec, axis=0).shape[0] == k
    c = hip.mfma_gemm_mx(a, lowp.e8m0(a_exp), b, lowp.e8m0(b_exp), fmt).numpy()
    want = np.ldexp(bdec[rows], a_exp[np.arange(m), rows // 32][:, None])
    assert np.array_equal(c, want.astype(np.float32))


# ---------------------------------------------------------------- exact GEMM
def _f64_product(a, b):
    import numpy as np
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("m,n,k", [(64, 64, 16), (128, 64, 80), (64, 192, 272)])
def test_fp8_gemm_is_exact_on_integer_data(m, n, k):
    import numpy as np
    from amdkube.ops import hip
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    a = rng.integers(-15, 16, (m, k)).astype(np.float32)
    b = rng.integers(-15, 16, (k, n)).astype(np.float32)
    assert np.array_equal(hip.mfma_gemm_fp8(a, b).numpy(), _f64_product(a, b))


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
@pytest.mark.parametrize("m,n,k", [(64, 64, 64), (128, 64, 192), (64, 192, 320)])
def test_mx_gemm_is_exact_on_code_data(fmt, m, n, k):
    """fp8: the integers -15..15; fp4: all 16 codes. With A scales from 2^-1, 1, 4 and B scales from
    2^-3, 1, 2 every partial sum is a multiple of 2^-4 (fp8) or 2^-6 (fp4) below 2^24 of them."""
    import numpy as np
    from amdkube.ops import hip, lowp
    rng = np.random.default_rng(1000 * m + 10 * n + k + (7 if fmt == "fp4" else 0))
    if fmt == "fp8":
        a, b = (lowp.encode_e4m3(rng.integers(-15, 16, s).astype(np.float32)) for s in ((m, k), (k, n)))
    else:
        a, b = (rng.integers(0, 16, s).astype(np.uint8) for s in ((m, k), (k, n)))
    sa = lowp.e8m0(rng.choice([-1, 0, 2], (m, k // 32)))
    sb = lowp.e8m0(rng.choice([-3, 0, 1], (k // 32, n)))
    assert len(np.unique(sa)) == 3 and len(np.unique(sb)) == 3
    want = _f64_product(lowp.mx_dequantize(a, sa, fmt, axis=1), lowp.mx_dequantize(b, sb, fmt, axis=0))
    assert np.array_equal(hip.mfma_gemm_mx(a, sa, b, sb, fmt).numpy(), want)


# ---------------------------------------------------------------- random data
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_random_data_within_the_fp32_summation_bound(dtype):
    import numpy as np
    import torch
    from amdkube.ops import hip, lowp
    m, n, k = 128, 128, 256
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(m, k, generator=g).numpy(), torch.randn(k, n, generator=g).numpy()
    if dtype == "fp8":
        a, b = lowp.decode_e4m3(lowp.encode_e4m3(a)), lowp.decode_e4m3(lowp.encode_e4m3(b))
        c = hip.mfma_gemm_fp8(a, b)
    else:
        fmt = dtype[2:]
        (qa, sa), (qb, sb) = lowp.mx_quantize(a, fmt, axis=1), lowp.mx_quantize(b, fmt, axis=0)
        a, b = lowp.mx_dequantize(qa, sa, fmt, axis=1), lowp.mx_dequantize(qb, sb, fmt, axis=0)
        c = hip.mfma_gemm_mx(qa, sa, qb, sb, fmt)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref = a64 @ b64
    bound = k * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64))
    cpu = (torch.from_numpy(a) @ torch.from_numpy(b)).numpy().astype(np.float64)     # torch's own fp32 matmul stays within it
    assert bool((np.abs(cpu - ref) <= bound).all())
    err = np.abs(c.numpy().astype(np.float64) - ref)
    print(f"mfma_gemm {dtype} max |err| / bound:", float((err / bound).max()))
    assert bool((err <= bound).all())


# ---------------------------------------------------------------- mfma_check
@pytest.fixture(scope="module")
def blocks():
    from amdkube.ops import hip
    return 4 * hip.device_info()["cu_count"]


@pytest.fixture(scope="module")
def tiles(blocks):
    from amdkube.ops import hip
    return {(dtype, blk, seed): tuple(x.numpy() for x in hip.mfma_check_tile(blk, seed=seed, dtype=dtype))
            for dtype in DTYPES for blk in (0, blocks - 1) for seed in (0x5EED, 12345)}


def _granularity(x, axis):
    """Per 32-block along `axis`: the largest power of two that divides every element."""
    import numpy as np
    v = np.moveaxis(x, axis, -1).reshape(64, -1, 32).astype(np.float64)
    g = np.full(v.shape[:2], 64.0)
    for _ in range(12):                                               # from 64 down to 2^-5
        g = np.where((np.mod(v, g[..., None]) != 0).any(-1), g / 2, g)
    return g


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_tile_operands_and_product(tiles, blocks, dtype):
    import numpy as np
    from amdkube.ops import lowp
    k = K_OF[dtype]
    for blk in (0, blocks - 1):
        for seed in (0x5EED, 12345):
            a, b, c = tiles[(dtype, blk, seed)]
            assert a.shape == (64, k) and b.shape == (k, 64) and c.shape == (64, 64)
            assert np.array_equal(c, _f64_product(a, b)), (dtype, blk, seed)
            for x, axis in ((a, 1), (b, 0)):
                if dtype == "fp8":                                    # the integers -15..15, all of them
                    assert np.array_equal(lowp.decode_e4m3(lowp.encode_e4m3(x)), x)
                    assert np.array_equal(np.unique(x), np.arange(-15, 16))
                else:                                                 # representable as codes times one scale per block
                    fmt = dtype[2:]
                    assert np.array_equal(lowp.mx_dequantize(*lowp.mx_quantize(x, fmt, axis), fmt, axis), x)
                    g = _granularity(x, axis)                         # 32 hashed codes: the block's unit shows its scale
                    assert len(np.unique(g)) >= 2, (dtype, blk, seed, np.unique(g))
                    units = np.moveaxis(x, axis, -1).reshape(64, -1, 32) / g[..., None]
                    assert len(np.unique(units)) == (31 if fmt == "fp8" else 15)   # the full code set


def test_check_tile_inputs_differ_by_seed_block_and_dtype(tiles, blocks):
    import numpy as np
    for dtype in DTYPES:
        for blk in (0, blocks - 1):
            for x in (0, 1):
                assert not np.array_equal(tiles[(dtype, blk, 0x5EED)][x], tiles[(dtype, blk, 12345)][x])
        for seed in (0x5EED, 12345):
            for x in (0, 1):
                assert not np.array_equal(tiles[(dtype, 0, seed)][x], tiles[(dtype, blocks - 1, seed)][x])
        a, b, _ = tiles[(dtype, 0, 0x5EED)]
        assert not np.array_equal(a[:, :64], b[:64, :])                                     # A is not B


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_clean_run(blocks, dtype):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, dtype=dtype)
    assert r["ok"] is True and r["errors"] == 0 and r["first_errors"] == [] and r["dtype"] == dtype
    assert r["blocks"] == blocks and r["rounds"] == 2 and r["k"] == K_OF[dtype]
    assert r["tflops"] > 0 and r["ms"] > 0 and "bf16_tflops" not in r


def test_check_bf16_keeps_its_keys_and_gains_dtype_and_tflops(blocks):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, dtype="bf16")
    assert r["ok"] is True and r["dtype"] == "bf16" and r["tflops"] == r["bf16_tflops"] > 0 and r["k"] == 128
    a, b, c = hip.mfma_check_tile(0, dtype="bf16")
    assert tuple(a.shape) == (64, 128) and tuple(c.shape) == (64, 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_selftest_flips_are_all_reported(blocks, dtype):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, selftest_flips=37, dtype=dtype)
    assert r["errors"] == 37 and r["ok"] is False and r["dtype"] == dtype
    recs = r["first_errors"]
    assert len(recs) == 16
    for e in recs:
        assert 0 <= e["block"] < blocks and 0 <= e["row"] < 64 and 0 <= e["col"] < 64 and e["round"] in (0, 1), e
        assert e["got"] != e["want"] and e["got"] ^ e["want"] == 1, e    # the low mantissa bit of the compared copy
    assert {e["round"] for e in recs} == {0, 1}
    assert len({(e["block"], e["row"], e["col"], e["round"]) for e in recs}) == 16


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_single_flip_single_round(dtype):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=1, selftest_flips=1, dtype=dtype)
    assert r["errors"] == 1 and r["ok"] is False and len(r["first_errors"]) == 1
    assert r["first_errors"][0]["round"] == 0


# ---------------------------------------------------------------- arguments
def test_bad_shapes_codes_and_dtypes_are_refused(blocks):
    import numpy as np
    from amdkube.ops import hip
    z = lambda *s: np.zeros(s, np.uint8)                              # noqa: E731
    with pytest.raises(ValueError):
        hip.mfma_gemm_fp8(np.zeros((32, 16), np.float32), np.zeros((16, 64), np.float32))   # M = 32
    with pytest.raises(ValueError):
        hip.mfma_gemm_fp8(np.zeros((64, 24), np.float32), np.zeros((24, 64), np.float32))   # K = 24
    with pytest.raises(ValueError):
        hip.mfma_gemm_fp8(np.zeros((64, 32), np.float32), np.zeros((16, 64), np.float32))   # inner dimensions differ
    for fmt in ("fp8", "fp4"):
        with pytest.raises(ValueError):
            hip.mfma_gemm_mx(z(64, 32), z(64, 1), z(32, 64), z(1, 64), fmt)                 # K = 32
        with pytest.raises(ValueError):
            hip.mfma_gemm_mx(z(64, 64), z(64, 1), z(64, 64), z(2, 64), fmt)                 # A scales are M x K/32
        with pytest.raises(ValueError):
            hip.mfma_gemm_mx(z(64, 64), z(64, 2), z(64, 96), z(2, 96), fmt)                 # N = 96
        with pytest.raises(ValueError):
            hip.mfma_gemm_mx(z(64, 64).astype(np.float32), z(64, 2), z(64, 64), z(2, 64), fmt)   # codes are uint8
    with pytest.raises(ValueError):
        hip.mfma_gemm_mx(z(64, 64) + 16, z(64, 2), z(64, 64), z(2, 64), "fp4")              # e2m1 codes end at 15
    with pytest.raises(ValueError):
        hip.mfma_gemm_mx(z(64, 64), z(64, 2), z(64, 64), z(2, 64), "fp6")
    with pytest.raises(ValueError):
        hip.mfma_check(rounds=1, dtype="fp6")
    with pytest.raises(ValueError):
        hip.mfma_check_tile(0, dtype="fp16")
    with pytest.raises(ValueError):
        hip.mfma_check_tile(blocks, dtype="mxfp4")                                          # outside the grid
