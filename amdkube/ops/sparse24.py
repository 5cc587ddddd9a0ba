"""The 2:4 structured-sparse format of the sparse matrix-core paths (kernels/mfma_check_sparse.h), in numpy.

A is M×K; in every aligned group of four consecutive k of a row at most two entries are non-zero. It
travels as `values` (M×K/2, the kept entries of each group in ascending k) and `meta` (M×K/32 uint32
words): group g of a row is bits 4(g mod 8).. of that row's word g // 8, bits 1:0 the position (0..3)
of the first kept value and bits 3:2 that of the second, the first strictly below the second. A group
with fewer than two non-zeros keeps zeros at its lowest free positions."""
from __future__ import annotations

import numpy as np

PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))   # the position pairs a group can keep
_SHIFTS = 4 * np.arange(8, dtype=np.uint32)


def _groups(a):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] == 0 or a.shape[1] % 32:
        raise ValueError(f"need a 2-D array whose K is a positive multiple of 32, got shape {a.shape}")
    return a.reshape(a.shape[0], a.shape[1] // 4, 4)


def compress(a):
    """(values, meta) of a 2:4-sparse `a`; ValueError on a group with three or more non-zeros."""
    g = _groups(a)
    nz = g != 0
    if (nz.sum(-1) > 2).any():
        i, j = np.argwhere(nz.sum(-1) > 2)[0]
        raise ValueError(f"not 2:4 sparse: row {i} has more than two non-zeros in k {4 * j}..{4 * j + 3}")
    # the non-zero positions first, then the free ones, each in ascending k; the first two, ascending
    pos = np.sort(np.argsort(~nz, axis=-1, kind="stable")[..., :2], axis=-1)
    values = np.take_along_axis(g, pos, -1).reshape(g.shape[0], -1)
    fields = (pos[..., 0] | pos[..., 1] << 2).astype(np.uint32).reshape(g.shape[0], -1, 8)
    return values, (fields << _SHIFTS).sum(-1, dtype=np.uint32)


def expand(values, meta, k: int):
    """The dense M×k matrix of `values` and `meta`."""
    values, meta = np.asarray(values), np.asarray(meta, dtype=np.uint32)
    m = values.shape[0]
    if values.shape != (m, k // 2) or meta.shape != (m, k // 32) or k % 32:
        raise ValueError(f"need values Mx{k // 2} and meta Mx{k // 32}, got {values.shape} and {meta.shape}")
    fields = ((meta[:, :, None] >> _SHIFTS) & 15).reshape(m, k // 4).astype(np.intp)
    v = values.reshape(m, k // 4, 2)
    out = np.zeros((m, k // 4, 4), values.dtype)
    np.put_along_axis(out, (fields & 3)[..., None], v[..., :1], -1)
    np.put_along_axis(out, (fields >> 2)[..., None], v[..., 1:], -1)
    return out.reshape(m, k)


def prune(a):
    """`a` with the two entries of largest magnitude of every group kept, the lower k on ties."""
    g = _groups(a)
    keep = np.argsort(-np.abs(g.astype(np.float64)), axis=-1, kind="stable")[..., :2]   # float: |int8 -128| too
    mask = np.zeros(g.shape, bool)
    np.put_along_axis(mask, keep, True, -1)
    return np.where(mask, g, 0).reshape(np.asarray(a).shape).astype(g.dtype)
