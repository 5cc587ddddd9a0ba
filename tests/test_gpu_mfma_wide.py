"""GPU tier: the matrix-core check on the FP64 and INT8 paths (kernels/mfma_check_wide.h:
v_mfma_f64_16x16x4_f64 and v_mfma_i32_32x32x32_i8) through mfma-check --dtype and the in-process ops.

The tests that start child processes come first and torch is imported inside the tests, as in
test_gpu_mfma_check.py. On integer data (fp64 |v| <= 2^23, int8 the full range) every partial sum is
exact in the accumulator, so the GEMM must equal the numpy int64 product; the one-hot tests pin the
operand and C/D lane maps. On real fp64 data the bound is K * 2^-52 * (|A| @ |B|) against a longdouble
product: any-order fused fp64 summation of K terms is within K * 2^-53 * sum|a b|, times the factor 2
that the bf16 and low-precision tests carry.
"""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
DTYPES, K_OF = ("fp64", "int8"), {"fp64": 32, "int8": 256}
SHAPES = {"fp64": [(64, 64, 4), (64, 128, 36), (128, 64, 68)], "int8": [(64, 64, 32), (64, 128, 160), (128, 64, 288)]}
CASES = [(d, *s) for d in DTYPES for s in SHAPES[d]]


def _check(*args):
    r = subprocess.run([os.path.join(BIN, "mfma-check"), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


def _gemm(dtype, a, b):
    from amdkube.ops import hip
    return (hip.mfma_gemm_fp64 if dtype == "fp64" else hip.mfma_gemm_int8)(a, b)


def _integers(dtype, shape, rng):
    import numpy as np
    lo, hi, t = (-2 ** 23, 2 ** 23 + 1, np.float64) if dtype == "fp64" else (-128, 128, np.int8)
    return rng.integers(lo, hi, shape).astype(t)


def test_binary_checks_both_wide_dtypes():
    rc, lines, r = _check("--dtype", "fp64,int8", "--rounds", "2")
    assert rc == 0 and [d["dtype"] for d in lines] == list(DTYPES), (r.stdout, r.stderr)
    for d in lines:
        assert d["errors"] == 0 and d["first_errors"] == [] and d["rounds"] == 2 and d["k"] == K_OF[d["dtype"]], d


def test_binary_reports_selftest_flips_on_int8():
    rc, lines, r = _check("--dtype", "int8", "--selftest-flips", "3", "--rounds", "1")
    assert rc == 1 and len(lines) == 1 and lines[0]["errors"] == 3, (r.stdout, r.stderr)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_picks_exact_rows_and_columns(dtype):
    import numpy as np
    m = 64 if dtype == "fp64" else 128                                # M = K: a permutation matrix
    perm = (np.arange(m) * 37 + 11) % m
    onehot = np.zeros((m, m), np.int64)
    onehot[np.arange(m), perm] = 1
    k, j = np.arange(m)[:, None], np.arange(m)[None, :]
    data = 1000 * k + j if dtype == "fp64" else ((37 * k + 11 * j) % 251) - 125
    assert np.unique(data, axis=0).shape[0] == m and np.unique(data, axis=1).shape[1] == m
    assert np.array_equal(_gemm(dtype, onehot, data).numpy(), data[perm])             # A picks rows of B
    assert np.array_equal(_gemm(dtype, data, onehot.T).numpy(), data[:, perm])         # B picks columns of A


@pytest.mark.parametrize("dtype,m,n,k", CASES)
def test_gemm_is_exact_on_integer_data(dtype, m, n, k):
    import numpy as np
    import torch
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    a, b = _integers(dtype, (m, k), rng), _integers(dtype, (k, n), rng)
    c = _gemm(dtype, a, b)
    assert c.dtype == (torch.float64 if dtype == "fp64" else torch.int32) and tuple(c.shape) == (m, n)
    assert np.array_equal(c.numpy().astype(np.int64), a.astype(np.int64) @ b.astype(np.int64))


@pytest.mark.parametrize("m,n,k", SHAPES["fp64"])
def test_fp64_gemm_on_real_data_within_the_fp64_summation_bound(m, n, k):
    import numpy as np
    rng = np.random.default_rng(7 + k)
    a, b = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    ref = a.astype(np.longdouble) @ b.astype(np.longdouble)
    bound = k * 2.0 ** -52 * (np.abs(a) @ np.abs(b))
    err = np.abs(_gemm("fp64", a, b).numpy().astype(np.longdouble) - ref).astype(np.float64)
    print(f"mfma_gemm_fp64 K={k} max |err| / bound:", float((err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_clean_run_and_tiles(dtype):
    import numpy as np
    import torch
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, dtype=dtype)
    assert r["ok"] is True and r["errors"] == 0 and r["dtype"] == dtype and r["k"] == K_OF[dtype] and r["tflops"] > 0
    seen = set()
    for blk in (0, r["blocks"] // 2, r["blocks"] - 1):
        a, b, c = hip.mfma_check_tile(blk, dtype=dtype)
        assert a.dtype == b.dtype == c.dtype == torch.float64
        assert tuple(a.shape) == (64, K_OF[dtype]) and tuple(b.shape) == (K_OF[dtype], 64) and tuple(c.shape) == (64, 64)
        a, b, c = (x.numpy().astype(np.int64) for x in (a, b, c))
        assert np.array_equal(a @ b, c), (dtype, blk)
        if dtype == "fp64":                                           # the operands use their range
            assert 2 ** 22 < max(np.abs(a).max(), np.abs(b).max()) <= 2 ** 23
        seen |= set(a.ravel().tolist()) | set(b.ravel().tolist())
    if dtype == "int8":
        assert seen == set(range(-128, 128))


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_selftest_flips_are_all_reported(dtype):
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, selftest_flips=5, dtype=dtype)
    recs = r["first_errors"]
    assert r["errors"] == 5 and r["ok"] is False and len(recs) == 5
    assert len({(e["block"], e["row"], e["col"]) for e in recs}) == 5
    assert all(e["round"] in (0, 1) and e["got"] != e["want"] and 0 <= e["row"] < 64 and 0 <= e["col"] < 64 for e in recs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_shapes_and_values_are_refused(dtype):
    import numpy as np
    k = 4 if dtype == "fp64" else 32
    z = lambda *s: np.zeros(s, np.float64)                            # noqa: E731
    for a, b in ((z(32, k), z(k, 64)), (z(64, k), z(k, 96)), (z(64, k // 2), z(k // 2, 64)), (z(64, 2 * k), z(k, 64)),
                 (z(64), z(k, 64))):                                  # M, N, K, the inner dimension, not 2-D
        with pytest.raises(ValueError):
            _gemm(dtype, a, b)
    if dtype == "int8":
        for bad in (128.0, -129.0, 0.5):
            with pytest.raises(ValueError):
                _gemm(dtype, z(64, k) + bad, z(k, 64))
