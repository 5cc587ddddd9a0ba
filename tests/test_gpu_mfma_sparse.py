"""GPU tier: the matrix-core check on the 2:4 sparse paths (kernels/mfma_check_sparse.h:
v_smfmac_f32_32x32x32_bf16 and v_smfmac_i32_32x32x64_i8) through mfma-check --dtype and the in-process ops.

Child processes first, torch imported inside the tests, as in test_gpu_mfma_check.py. A one-hot A pins the
place of B's values and the index decode, a one-hot B the place of A's values and their index slots; the data
is the % 251 pattern for both dtypes, since 1000 k + j is not exact in bf16. On integer data (sp-bf16 |v| <= 8)
every partial sum is exact. K = 32 / 64 is one instruction, a lone abid:0; the other shapes are full slices of
128 and a ragged one of an odd step count, (64, 64, 192) of an even one. On real bf16 data the bound is that of
test_gpu_mfma_check.py with K/2 products."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "amdkube", "_native", "bin")
DTYPES, K_OF = ("sp-bf16", "sp-int8"), {"sp-bf16": 128, "sp-int8": 256}
SHAPES = {"sp-bf16": [(64, 64, 32), (64, 128, 160), (128, 64, 288), (64, 64, 192)],
          "sp-int8": [(64, 64, 64), (64, 128, 192), (128, 64, 320)]}


def _check(*args):
    r = subprocess.run([os.path.join(BIN, "mfma-check"), *args], capture_output=True, text=True, timeout=120)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines()], r


def _gemm(dtype, a, b):
    from amdkube.ops import hip
    return hip.mfma_gemm_sparse(a, b, dtype=dtype)


def test_binary_checks_both_sparse_dtypes_and_reports_selftest_flips():
    rc, lines, r = _check("--dtype", "sp-bf16,sp-int8", "--rounds", "2")
    assert rc == 0 and [d["dtype"] for d in lines] == list(DTYPES), (r.stdout, r.stderr)
    for d in lines:
        assert d["errors"] == 0 and d["first_errors"] == [] and d["rounds"] == 2 and d["k"] == K_OF[d["dtype"]], d
    rc, lines, r = _check("--dtype", "sp-int8", "--selftest-flips", "3", "--rounds", "1")
    assert rc == 1 and len(lines) == 1 and lines[0]["errors"] == 3, (r.stdout, r.stderr)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_picks_exact_rows_and_columns(dtype):
    import numpy as np
    from amdkube.ops import sparse24
    m = 128                                                           # M = K: a permutation matrix, trivially 2:4
    perm = (np.arange(m) * 37 + 11) % m
    onehot = np.eye(m, dtype=np.int64)[perm]
    k, j = np.arange(m)[:, None], np.arange(m)[None, :]
    data = ((37 * k + 11 * j) % 251) - 125                            # asymmetric, rows and columns distinct
    assert np.array_equal(_gemm(dtype, onehot, data).numpy(), data[perm])             # A picks rows of B
    i, g = np.arange(m)[:, None], np.arange(m // 4)[None, :]                          # group g of row i: pair (i + g) % 6
    pos = np.array(sparse24.PAIRS)[(i + g) % 6]
    a = np.zeros((m, m // 4, 4), np.int64)
    np.put_along_axis(a, pos[..., :1], (1 + (7 * i + 3 * g) % 120)[..., None], -1)
    np.put_along_axis(a, pos[..., 1:], -(1 + (3 * i + 5 * g) % 120)[..., None], -1)
    a = a.reshape(m, m)
    assert np.array_equal(_gemm(dtype, a, onehot.T).numpy(), a[:, perm])               # B picks columns of A


@pytest.mark.parametrize("dtype,m,n,k", [(d, *s) for d in DTYPES for s in SHAPES[d]])
def test_gemm_is_exact_on_pruned_integer_data(dtype, m, n, k):
    import numpy as np
    import torch
    from amdkube.ops import sparse24
    rng = np.random.default_rng(1000 * m + 10 * n + k)
    lo, hi = (-8, 9) if dtype == "sp-bf16" else (-128, 128)
    a, b = sparse24.prune(rng.integers(lo, hi, (m, k))), rng.integers(lo, hi, (k, n))
    c = _gemm(dtype, a, b)
    assert c.dtype == (torch.float32 if dtype == "sp-bf16" else torch.int32) and tuple(c.shape) == (m, n)
    assert np.array_equal(c.numpy().astype(np.int64), a @ b)


@pytest.mark.parametrize("m,n,k", SHAPES["sp-bf16"])
def test_sp_bf16_gemm_on_real_data_within_the_fp32_summation_bound(m, n, k):
    import torch
    from amdkube.ops import sparse24
    g = torch.Generator().manual_seed(7 + k)
    a = torch.from_numpy(sparse24.prune(torch.randn(m, k, generator=g).numpy())).to(torch.bfloat16).double()
    b = torch.randn(k, n, generator=g).to(torch.bfloat16).double()
    bound = k / 2 * 2.0 ** -23 * (a.abs() @ b.abs())
    err = (_gemm("sp-bf16", a, b).double() - a @ b).abs()
    print(f"mfma_gemm_sparse sp-bf16 K={k} max |err| / bound:", float((err / bound.clamp_min(1e-300)).max()))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_clean_run_and_tiles(dtype):
    import numpy as np
    import torch
    from amdkube.ops import hip
    r = hip.mfma_check(rounds=2, dtype=dtype)
    assert r["ok"] is True and r["errors"] == 0 and r["dtype"] == dtype and r["k"] == K_OF[dtype] and r["tflops"] > 0
    pairs = []
    for blk in (0, r["blocks"] // 2, r["blocks"] - 1):
        a, b, c = hip.mfma_check_tile(blk, dtype=dtype)
        assert a.dtype == c.dtype == torch.float64 and tuple(a.shape) == (64, K_OF[dtype]) and tuple(c.shape) == (64, 64)
        a, b, c = (x.numpy().astype(np.int64) for x in (a, b, c))
        assert np.array_equal(a @ b, c), (dtype, blk)
        nz = a.reshape(-1, 4) != 0
        assert nz.sum(1).max() == 2
        pairs.append(nz[nz.sum(1) == 2] @ np.array([1, 2, 4, 8]))     # the groups with two products, by their positions
    masks, counts = np.unique(np.concatenate(pairs), return_counts=True)
    assert masks.tolist() == [3, 5, 6, 9, 10, 12] and counts.min() >= 2, (masks, counts)


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
    from amdkube.ops import hip
    k = K_OF[dtype] // 4                                              # one step: 32 / 64
    z = lambda *s: np.zeros(s, np.float64)                            # noqa: E731
    three = z(64, k)
    three[5, 8:11] = 1.0                                              # three non-zeros in one group
    for a, b in ((z(32, k), z(k, 64)), (z(64, k), z(k, 96)), (z(64, k // 2), z(k // 2, 64)), (z(64, 2 * k), z(k, 64)),
                 (three, z(k, 64))):                                  # M, N, K, the inner dimension, not 2:4
        with pytest.raises(ValueError):
            _gemm(dtype, a, b)
    if dtype == "sp-int8":
        for bad in (128.0, -129.0, 0.5):
            with pytest.raises(ValueError):
                _gemm(dtype, z(64, k), z(k, 64) + bad)
    with pytest.raises(ValueError, match="sp-fp16"):
        hip.mfma_gemm_sparse(z(64, k), z(k, 64), dtype="sp-fp16")
