"""The five streaming kernels behind "Test PASSED" and "Healthy", bit for bit against numpy and torch on
the CPU: vadd_kernel, the two kernels of hsa-vector-add's code object (amdkube_vadd, amdkube_copy), and
the HBM probe's write, verify, read and copy. The tests choose the grid, so that a few KiB reach what the
production grid reaches only at tens of MiB: the 8-deep main loops, a wave split between main loop and
tail, ragged and empty chunks. tests/stream_ref.py has the shapes and the reference;
tests/test_stream_shapes.py shows on the CPU that each shape reaches what it is there for.

In-process HIP only, no child processes, no tolerances."""
import functools

import numpy as np
import pytest

from tests import stream_ref as sr

pytestmark = pytest.mark.gpu

SEEDS = (0x5EED, 0xC0FFEE11)
FLT_MAX = np.finfo(np.float32).max


@functools.lru_cache(maxsize=None)
def cus():
    from amdkube.ops import hip
    return hip.device_info(0)["cu_count"]


@functools.lru_cache(maxsize=None)
def random_words(n16):
    w = np.random.default_rng(n16).integers(0, 1 << 32, 4 * n16, dtype=np.uint64).astype(np.uint32)
    w.setflags(write=False)
    return w


# ---------------------------------------------------------------------------- HBM write
@pytest.mark.parametrize("shape", sr.WRITE_SHAPES, ids=sr.shape_id)
def test_write_is_the_pattern(shape):
    from amdkube.ops import hip
    n16, grid, _ = shape
    for seed in SEEDS:
        got = hip.hbm_pattern(n16, seed, grid=grid)
        assert got.dtype == np.uint32 and np.array_equal(got, sr.pattern(n16, seed)), (shape, hex(seed))


# ---------------------------------------------------------------------------- HBM verify
def flipped(n16, launched):
    """The pattern with one bit flipped in one 32-bit word of every edge item and in 20 other words."""
    rng = np.random.default_rng(4 * n16 + 1)
    words = {4 * i + int(rng.integers(4)) for i in sr.edge_items(n16, launched)}
    others = np.setdiff1d(np.arange(4 * n16), sorted(words))
    words |= set(rng.choice(others, min(20, others.size), replace=False).tolist())
    bad = sr.pattern(n16, SEEDS[0]).copy()
    for w in words:
        bad[w] ^= np.uint32(1) << np.uint32(rng.integers(32))
    return bad, len(words)


@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
def test_verify_counts_every_flipped_word_once(shape):
    from amdkube.ops import hip
    n16, grid, _ = shape
    for seed in SEEDS:
        assert hip.hbm_verify(sr.pattern(n16, seed), seed, grid=grid) == 0, (shape, hex(seed))
    bad, count = flipped(n16, sr.chunked_grid(n16, grid, cus()))
    assert count >= min(4 * n16, 21)
    # a skipped item loses its flip, an item visited twice counts it twice
    assert hip.hbm_verify(bad, SEEDS[0], grid=grid) == count, shape
    # against the other seed's pattern (nearly) every word differs: the count is that of the whole range
    differing = int((bad != sr.pattern(n16, SEEDS[1])).sum())
    assert differing >= 4 * n16 - 1 and hip.hbm_verify(bad, SEEDS[1], grid=grid) == differing, shape


# ---------------------------------------------------------------------------- HBM copy
@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
def test_copy_returns_every_word(shape):
    """The destination holds 0xff bytes before the launch (hbm_copy_host), so a store that was skipped
    cannot pass on stale data."""
    from amdkube.ops import hip
    n16, grid, _ = shape
    src = random_words(n16)
    got = hip.hbm_copy(src, grid=grid)
    assert got.dtype == np.uint32 and np.array_equal(got, src), shape


def test_copy_destination_is_prefilled():
    """... which this shows: nothing is copied from an empty source, and zeros come back as zeros."""
    from amdkube.ops import hip
    assert hip.hbm_copy(np.zeros(0, np.uint32)).size == 0
    assert np.array_equal(hip.hbm_copy(np.zeros(4 * 2049, np.uint32), grid=1), np.zeros(4 * 2049, np.uint32))


# ---------------------------------------------------------------------------- HBM read
def read_positions(n16, launched):
    """First, last, 107 and 108 of a 1900-item chunk, 2047 and 2048."""
    edge = sr.edge_items(n16, launched)
    firsts_lasts = {i for lo, hi in sr.chunks(n16, launched) if lo < hi for i in (lo, hi - 1)}
    return sorted({0, n16 - 1} | (set(edge) - firsts_lasts))


@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
def test_read_loads_every_edge_item(shape):
    from amdkube.ops import hip
    n16, grid, _ = shape
    buf = np.zeros(4 * n16, np.uint32)
    assert hip.hbm_read(buf, grid=grid) == 0, shape
    positions = read_positions(n16, sr.chunked_grid(n16, grid, cus()))
    if (n16, grid) == (3800, 2):
        assert positions == [0, 107, 108, 2007, 2008, 2047, 2048, 3799]
    for k, item in enumerate(positions):
        buf[:] = 0
        buf[4 * item + k % 4] = sr.READ_MAGIC
        assert hip.hbm_read(buf, grid=grid) == sr.READ_MAGIC, (shape, item)


# ---------------------------------------------------------------------------- the vector adds
def normal_floats(n, seed):
    """Random fp32 over 40 binades, no subnormals in or out: a sum is a multiple of the smaller
    operand's ulp, far above 2^-126 here."""
    import torch
    g = torch.Generator().manual_seed(seed)
    scale = torch.pow(2.0, torch.randint(-20, 21, (n,), generator=g).float())
    return torch.randn(n, generator=g) * scale


# exact in fp32, the sign of zero included: infinities, zeros of both signs, x + (-x), overflow to infinity
FIXED_A = np.array([np.inf, -np.inf, np.inf, -np.inf, 0.0, -0.0, 0.0, -0.0, 1.5, -3.25e7, FLT_MAX, -FLT_MAX, FLT_MAX], np.float32)
FIXED_B = np.array([1.0, 1.0, np.inf, -np.inf, 0.0, -0.0, -0.0, 0.0, -1.5, 3.25e7, FLT_MAX, -FLT_MAX, -FLT_MAX], np.float32)
# every sum is NaN: a NaN operand (quiet, signalling, negative) or inf - inf
NAN_A = np.array([0x7FC00000, 0x3F800000, 0x7F800001, 0x7F800000, 0xFF800000, 0xFFFFFFFF], np.uint32).view(np.float32)
NAN_B = np.array([0x3F800000, 0xFFC00000, 0x40000000, 0xFF800000, 0x7F800000, 0x7FC00000], np.uint32).view(np.float32)


def check_vector_add(add, n):
    """`add(a, b)` (float32 numpy in and out) against torch on the CPU."""
    import torch
    a, b = normal_floats(n, 2 * n + 1), normal_floats(n, 2 * n + 2)
    want = (a + b).numpy()
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) >= np.finfo(np.float32).tiny).all()
    got = add(a.numpy(), b.numpy())
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), n
    # the fixed vector, tiled over the whole range so that vector body and scalar tail both see it
    a, b = np.resize(FIXED_A, n), np.resize(FIXED_B, n)
    want = (torch.from_numpy(a) + torch.from_numpy(b)).numpy()
    assert not np.isnan(want).any()
    assert np.array_equal(add(a, b).view(np.uint32), want.view(np.uint32)), n
    assert np.isnan(add(np.resize(NAN_A, n), np.resize(NAN_B, n))).all(), n


def test_fixed_vector_is_what_it_says():
    with np.errstate(all="ignore"):
        want, nans = FIXED_A + FIXED_B, NAN_A + NAN_B
    assert np.array_equal(want.view(np.uint32), np.array(
        [np.inf, -np.inf, np.inf, -np.inf, 0.0, -0.0, 0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, 0.0], np.float32).view(np.uint32))
    assert np.isnan(NAN_A).any(axis=0) and np.isnan(nans).all()


@pytest.mark.parametrize("shape", sr.VADD_SHAPES, ids=sr.shape_id)
def test_vadd_kernel_is_bit_equal_to_torch(shape):
    import torch
    from amdkube.ops import hip
    n, grid, _ = shape
    check_vector_add(lambda a, b: hip.vector_add_tensors(torch.from_numpy(a), torch.from_numpy(b), grid=grid).numpy(), n)


CO_SHAPES = [s for s in sr.VADD_SHAPES if s[1]]     # the code-object kernels always get a number of groups


@pytest.mark.parametrize("shape", CO_SHAPES, ids=sr.shape_id)
def test_amdkube_vadd_is_bit_equal_to_torch(shape):
    from amdkube.ops import hip
    n, groups, _ = shape
    check_vector_add(lambda a, b: hip.hsa_vadd_arrays(a, b, groups), n)


@pytest.mark.parametrize("shape", CO_SHAPES, ids=sr.shape_id)
def test_amdkube_copy_returns_every_bit(shape):
    from amdkube.ops import hip
    n, groups, _ = shape
    src = random_words((n + 3) // 4)[:n].copy()
    src[::5] = np.resize(NAN_A.view(np.uint32), src[::5].size)       # NaN patterns among them
    got = hip.hsa_copy_array(src.view(np.float32), groups)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), src), shape


# ---------------------------------------------------------------------------- bad grids
def test_bad_grids_are_refused():
    import torch
    from amdkube.ops import hip
    words, one = np.zeros(4, np.uint32), np.ones(4, np.float32)
    for grid in (-1, 65537):
        for call in (lambda: hip.hbm_pattern(1, grid=grid), lambda: hip.hbm_verify(words, grid=grid),
                     lambda: hip.hbm_copy(words, grid=grid), lambda: hip.hbm_read(words, grid=grid),
                     lambda: hip.vector_add_tensors(torch.ones(4), torch.ones(4), grid=grid)):
            with pytest.raises(ValueError):
                call()
    for groups in (0, -1, 65537):
        with pytest.raises(ValueError):
            hip.hsa_vadd_arrays(one, one, groups)
        with pytest.raises(ValueError):
            hip.hsa_copy_array(one, groups)
    assert hip.hbm_verify(sr.pattern(1, SEEDS[0]), SEEDS[0], grid=65536) == 0      # the largest grid allowed
