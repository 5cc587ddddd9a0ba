"""The numpy reference of the lane check (amdkube/ops/lanecheck.py) against a naive loop over the lanes of a
wave that moves the values the way each control is documented to, and kernels/lane_plan.h through its
stand-alone self-test, built plain and with ASan/UBSan (native/lane_plan_selftest.cpp says what it checks).
CPU tier."""
import os
import subprocess
import sys

import pytest

from amdkube.ops import lanecheck as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amdkube", "_native", "bin")
sys.path.insert(0, os.path.join(ROOT, "native"))


@pytest.fixture(scope="module", autouse=True)
def built():
    import build as nb
    nb.build(sanitize=True, cpu_only=True, jobs=4)


@pytest.mark.parametrize("binary", ["lane-plan-selftest", "lane-plan-selftest-asan"])
def test_lane_plan_selftest(binary):
    r = subprocess.run([os.path.join(BIN, binary)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def _naive_dpp(ctrl, l):
    """The lane that DPP control `ctrl` reads for lane l, or None where it has no source."""
    row, r, n = l // 16, l % 16, ctrl % 16
    if ctrl < 0x100:
        return 4 * (l // 4) + [(ctrl >> s) & 3 for s in (0, 2, 4, 6)][l % 4]
    if ctrl < 0x130:
        kind = (ctrl >> 4) & 3                                   # row_shl, row_shr, row_ror
        pos = r + n if kind == 0 else r - n if kind == 1 else (r - n) % 16
        return 16 * row + pos if 0 <= pos < 16 else None
    return {0x130: l + 1 if l < 63 else None, 0x134: (l + 1) % 64, 0x138: l - 1 if l else None, 0x13C: (l - 1) % 64,
            0x140: 16 * row + 15 - r, 0x141: 8 * (l // 8) + 7 - l % 8, 0x142: 16 * row - 1 if row else None,
            0x143: 31 if row >= 2 else None}[ctrl]


@pytest.mark.parametrize("entry", lc.DPP_TABLE, ids=lambda e: f"{e[0]:#x}-{e[1]:x}-{e[2]:x}-{int(e[3])}")
def test_dpp_source_lanes_against_a_loop_over_the_lanes(entry):
    ctrl, row_mask, bank_mask, bound = entry
    want = []
    for l in range(64):
        if not (row_mask >> (l // 16)) & 1 or not (bank_mask >> (l % 16 // 4)) & 1:
            want.append(lc.SRC_OLD)
            continue
        s = _naive_dpp(ctrl, l)
        want.append(s if s is not None else lc.SRC_ZERO if bound else lc.SRC_OLD)
    assert lc.dpp_src(entry).tolist() == want


def test_the_table_takes_every_control_both_ways_and_the_tables_have_their_shapes():
    assert len(lc.DPP_TABLE) == 40 and {e[:3] for e in lc.DPP_TABLE[:19]} == {e[:3] for e in lc.DPP_TABLE[19:38]}
    assert [e[3] for e in lc.DPP_TABLE[:38]] == [False] * 19 + [True] * 19
    assert lc.dpp_table(1, 0).shape == (1024, 45) and lc.perm_table(1, 0).shape == (1024, 13)
    assert lc.tr_registers(1, 0).shape == (1024, 9) and lc.dma_image(1, 0).shape == (40960,)


@pytest.mark.parametrize("width", [16, 32])
def test_the_swaps_exchange_the_documented_halves(width):
    a, b = list(range(64)), list(range(100, 164))               # (vdst, src0) before the swap
    for lo in range(0, 64, 2 * width):                          # A's upper part and B's lower part change places
        a[lo + width:lo + 2 * width], b[lo:lo + width] = b[lo:lo + width], a[lo + width:lo + 2 * width]
    for reg, after in ((0, a), (1, b)):
        which, lane = lc.swap_src(width, reg)
        assert [100 * int(w) + int(l) for w, l in zip(which, lane)] == after


@pytest.mark.parametrize("offset", lc.SWIZZLE, ids=hex)
def test_swizzle_source_lanes(offset):
    want = []
    for l in range(64):
        if offset & 0x8000:
            want.append(4 * (l // 4) + ((offset >> 2 * (l % 4)) & 3))
        else:
            a, o, x = offset & 31, (offset >> 5) & 31, (offset >> 10) & 31
            want.append(32 * (l // 32) + (((l % 32 & a) | o) ^ x))
    assert lc.swizzle_src(offset).tolist() == want


@pytest.mark.parametrize("form", range(4), ids=lc.TR_FORMS)
def test_each_transpose_map_permutes_the_elements_of_its_16_rows(form):
    per = lc.TR_PER_LANE[form]
    for blk in range(4):
        got = sorted(int(lc.tr_element(form, l, j)) for l in range(16 * blk, 16 * blk + 16) for j in range(per))
        assert got == list(range(16 * blk * per, 16 * (blk + 1) * per))
