"""CPU tier: the 2:4 sparse format in numpy (amdkube/ops/sparse24.py), which the sparse matrix-core GEMM
takes its operands from, and the device plugin's dtype list with the two sparse names."""
import numpy as np
import pytest

from amdkube.ops import sparse24


def _every_pair_with(count):   # one row of 32 k per position pair: `count` non-zeros a group, at the pair's positions
    a = np.zeros((6, 8, 4), np.float32)
    for i, (p, q) in enumerate(sparse24.PAIRS):
        a[i, :, [p, q][:count]] = np.arange(1, 8 * count + 1, dtype=np.float32).reshape(count, 8)
    return a.reshape(6, 32)


@pytest.mark.parametrize("a", [sparse24.prune(np.random.default_rng(3).standard_normal((8, 96)).astype(np.float32)),
                               sparse24.prune(np.random.default_rng(4).integers(-128, 128, (4, 64))),
                               _every_pair_with(0), _every_pair_with(1), _every_pair_with(2)])
def test_expand_undoes_compress(a):
    values, meta = sparse24.compress(a)
    k = a.shape[1]
    assert values.shape == (a.shape[0], k // 2) and meta.shape == (a.shape[0], k // 32) and meta.dtype == np.uint32
    fields = (meta[:, :, None] >> (4 * np.arange(8))) & 15
    assert ((fields & 3) < (fields >> 2)).all()
    assert np.array_equal(sparse24.expand(values, meta, k), a)


def test_metadata_word_layout_on_a_hand_written_row():
    row = np.zeros(64, np.int64)
    row[[1, 2]] = 5, 6          # group 0: positions 1, 2 -> field 0x9
    row[7] = 7                  # group 1: position 3, padded at the free position 0 -> field 0xC, values 0, 7
    row[[28, 31]] = 8, 9        # group 7: positions 0, 3 -> field 0xC in bits 28..31
    row[[34, 35]] = -1, -2      # group 8: positions 2, 3 -> field 0xE in bits 0..3 of word 1
    values, meta = sparse24.compress(row[None, :])
    assert meta.tolist() == [[0xC44444C9, 0x4444444E]]                # an empty group keeps positions 0, 1: field 0x4
    assert values[0, :4].tolist() == [5, 6, 0, 7] and values[0, 14:18].tolist() == [8, 9, -1, -2]


def test_compress_refuses_three_non_zeros():
    a = np.zeros((2, 32))
    a[1, 4:7] = 1
    with pytest.raises(ValueError, match="row 1 .* k 4..7"):
        sparse24.compress(a)


def test_prune_keeps_the_two_largest_and_the_lower_k_on_ties():
    a = np.tile(np.array([[1.0, -3.0, 2.0, 0.5, 2.0, -2.0, 2.0, 1.0]]), (1, 4))
    assert sparse24.prune(a)[0, :8].tolist() == [0, -3.0, 2.0, 0, 2.0, -2.0, 0, 0]
    assert sparse24.prune(np.full((1, 32), -128, np.int8)).reshape(8, 4).tolist() == [[-128, -128, 0, 0]] * 8


def test_the_plugin_takes_the_sparse_dtypes():
    from amdkube.cmd.components import device_plugin_parser
    from amdkube.deviceplugin import amd
    assert amd.parse_mfma_check_dtype("fp64,sp-bf16,sp-int8") == "fp64,sp-bf16,sp-int8"
    for bad in ("sp-fp16", "fp16"):
        with pytest.raises(ValueError):
            amd.parse_mfma_check_dtype(bad)
    assert device_plugin_parser().parse_args(["--mfma-check-dtype", "sp-int8"]).mfma_check_dtype == "sp-int8"
