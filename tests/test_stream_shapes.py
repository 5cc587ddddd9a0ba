"""The shapes of tests/test_gpu_stream_kernels.py mean what their table rows say. A model of each
streaming kernel's index arithmetic (tests/stream_ref.py) is run on the CPU for every shape: it must
visit every index exactly once, and the shape must have the property it was chosen for, such as a wave
with lanes on both sides of the main-loop condition or a workgroup with an empty chunk. If a constant
such as HBM_UNROLL changes, this fails before the GPU tests quietly stop reaching the loops they are for."""
import collections
import os
import re

import pytest

from tests import stream_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_those_of_the_headers():
    src = open(os.path.join(ROOT, "kernels", "gpu_common.h")).read() + open(os.path.join(ROOT, "kernels", "vadd_contract.h")).read()

    def const(name):
        return int(re.search(r"constexpr (?:int|unsigned) %s = (\d+);" % name, src).group(1))
    assert {n: const(n) for n in ("HBM_UNROLL", "HBM_WRITE_UNROLL", "HBM_BLOCKS_PER_CU", "HBM_COPY_BLOCKS_PER_CU",
                                  "VADD_BLOCKS_PER_CU", "VADD_WG")} == {
        "HBM_UNROLL": sr.HBM_UNROLL, "HBM_WRITE_UNROLL": sr.HBM_WRITE_UNROLL, "HBM_BLOCKS_PER_CU": sr.HBM_BLOCKS_PER_CU,
        "HBM_COPY_BLOCKS_PER_CU": sr.HBM_COPY_BLOCKS_PER_CU, "VADD_BLOCKS_PER_CU": sr.VADD_BLOCKS_PER_CU, "VADD_WG": sr.VADD_WG}
    # every HBM kernel is bounded to, and launched with, 256 lanes
    for kernel in ("hbm_write_kernel", "hbm_verify_kernel", "hbm_read_kernel", "hbm_copy_kernel"):
        assert re.search(r"__launch_bounds__\(%d\) void %s\b" % (sr.BLOCK, kernel), src), kernel
        assert re.search(r"hipLaunchKernelGGL\(%s, dim3\(\w+\), dim3\(%d\)" % (kernel, sr.BLOCK), src), kernel
    assert "0x%08xu" % sr.READ_MAGIC in src
    assert sr.stream_grid(0, 256, 64) == 1 and sr.stream_grid(257, 256, 64) == 2 and sr.stream_grid(1 << 40, 0, 64) == 16384
    assert sr.write_front_grid(256) == 128 and sr.write_front_grid(1) == 1


def test_readme_names_the_files_that_exist():
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("test_gpu_stream_kernels.py", "test_stream_shapes.py", "stream_ref.py"):
        assert "`%s`" % name in readme and os.path.exists(os.path.join(ROOT, "tests", name)), name


def exactly_once(visits, n):
    seen = collections.Counter(v[0] for v in visits)
    assert sorted(seen) == list(range(n)), "the union of visited indices is not range(n)"
    assert set(seen.values()) <= {1}, [i for i, c in seen.items() if c != 1][:8]


def iterations(visits, grid, lanes):
    """(workgroup, lane) -> {"main": iterations, "tail": iterations, ...}, idle lanes included."""
    per = {(b, t): collections.Counter() for b in range(grid) for t in range(lanes)}
    for _, blk, t, phase, it in visits:
        per[blk, t][phase] = max(per[blk, t][phase], it + 1)
    return per


def split_waves(per, phase):
    """Waves with lanes that take `phase` and lanes that do not."""
    waves = collections.defaultdict(set)
    for (blk, t), c in per.items():
        waves[blk, t // sr.WAVE].add(c[phase] > 0)
    return [w for w, s in waves.items() if len(s) == 2]


# ---------------------------------------------------------------------------- verify, read, copy
def one_main_full_tail_partial_tail(n16, grid, per):
    assert [hi - lo for lo, hi in sr.chunks(n16, grid)] == [2334, 2334, 2332]
    assert all(c["main"] == 1 for c in per.values())
    tails = collections.Counter(c["tail"] for c in per.values())
    assert set(tails) == {1, 2}                       # a pass all lanes make, then one only some make


def main_loop_splits_a_wave(n16, grid, per):
    assert [hi - lo for lo, hi in sr.chunks(n16, grid)] == [1900, 1900]
    for blk in range(grid):
        assert [t for t in range(sr.BLOCK) if per[blk, t]["main"]] == list(range(108))
        assert all(per[blk, t]["tail"] for t in range(108, sr.BLOCK))
    assert sorted(split_waves(per, "main")) == [(0, 1), (1, 1)]


def main_only(n16, grid, per):
    assert all(c["main"] == 1 and c["tail"] == 0 for c in per.values())


def main_plus_one_lane_tail(n16, grid, per):
    assert all(c["main"] == 1 for c in per.values())
    assert [k for k, c in per.items() if c["tail"]] == [(0, 0)] and per[0, 0]["tail"] == 1


def empty_chunk(n16, grid, per):
    lo, hi = sr.chunks(n16, grid)[-1]
    assert lo > n16 and hi == n16                     # past the end, not merely at it
    assert not any(per[grid - 1, t] for t in range(sr.BLOCK))


def single_item(n16, grid, per):
    assert [k for k, c in per.items() if c] == [(0, 0)]


def production_tail_only(n16, grid, per):
    assert grid == 257 and not any(c["main"] for c in per.values())


CHUNKED_PROPERTIES = {f.__name__: f for f in (one_main_full_tail_partial_tail, main_loop_splits_a_wave, main_only,
                                             main_plus_one_lane_tail, empty_chunk, single_item, production_tail_only)}


@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
@pytest.mark.parametrize("per_cu", [sr.HBM_BLOCKS_PER_CU, sr.HBM_COPY_BLOCKS_PER_CU], ids=["verify_read", "copy"])
def test_chunked_shape_covers_its_range_and_has_its_property(shape, per_cu):
    n16, grid, prop = shape
    grid = sr.chunked_grid(n16, grid, per_cu=per_cu)
    visits = sr.chunked_visits(n16, grid)
    exactly_once(visits, n16)
    CHUNKED_PROPERTIES[prop](n16, grid, iterations(visits, grid, sr.BLOCK))


def test_edge_items_are_where_the_loops_change():
    assert sr.edge_items(3800, 2) == [0, 107, 108, 1899, 1900, 2007, 2008, 2047, 2048, 3799]
    assert sr.edge_items(7000, 3) == [0, 2047, 2048, 2333, 2334, 4667, 4668, 6999]
    assert sr.edge_items(2048, 1) == [0, 2047] and sr.edge_items(2049, 1) == [0, 2047, 2048]
    assert sr.edge_items(5, 4) == [0, 1, 2, 3, 4] and sr.edge_items(1, 1) == [0]
    # 107 is the last lane of a 1900-item chunk in the main loop, 108 the first that is not
    per = iterations(sr.chunked_visits(3800, 2), 2, sr.BLOCK)
    assert per[0, 107]["main"] and not per[0, 108]["main"]


# ---------------------------------------------------------------------------- write
def w_one_main_partial_tail(n16, grid, per):
    assert all(c["main"] == 1 for c in per.values())
    assert {c["tail"] for c in per.values()} == {0, 1}


def w_main_loop_splits_a_wave(n16, grid, per):
    lanes = [blk * sr.BLOCK + t for (blk, t), c in sorted(per.items()) if c["main"]]
    assert lanes == list(range(388))
    assert split_waves(per, "main") == [(1, 2)]       # global lane 388 is lane 132 of workgroup 1


def w_main_only(n16, grid, per):
    main_only(n16, grid, per)


def w_main_plus_one_lane_tail(n16, grid, per):
    main_plus_one_lane_tail(n16, grid, per)


def w_most_lanes_idle(n16, grid, per):
    assert sorted(k for k, c in per.items() if c) == [(0, t) for t in range(5)]
    assert not any(c["main"] for c in per.values())


def w_single_item(n16, grid, per):
    single_item(n16, grid, per)


def w_production(n16, grid, per):
    assert grid == 128 and all(c["main"] == 1 for c in per.values())


WRITE_PROPERTIES = {f.__name__[2:]: f for f in (w_one_main_partial_tail, w_main_loop_splits_a_wave, w_main_only,
                                               w_main_plus_one_lane_tail, w_most_lanes_idle, w_single_item, w_production)}


@pytest.mark.parametrize("shape", sr.WRITE_SHAPES, ids=sr.shape_id)
def test_write_shape_covers_its_range_and_has_its_property(shape):
    n16, grid, prop = shape
    grid = sr.write_grid(grid)
    visits = sr.write_visits(n16, grid)
    exactly_once(visits, n16)
    WRITE_PROPERTIES[prop](n16, grid, iterations(visits, grid, sr.BLOCK))


# ---------------------------------------------------------------------------- the vector adds and amdkube_copy
def v_ten_ragged_iterations_three_scalars(n, grid, per):
    assert n // 4 == 7000 and {c["vec"] for c in per.values()} == {9, 10}
    assert [k for k, c in sorted(per.items()) if c["scalar"]] == [(0, 0), (0, 1), (0, 2)]


def v_one_wave_per_chunk_and_scalars(n, grid, per):
    for blk in range(grid):
        assert [t for t in range(sr.VADD_WG) if per[blk, t]["vec"]] == list(range(sr.WAVE))
    assert [k for k, c in sorted(per.items()) if c["scalar"]] == [(0, 0), (0, 1), (0, 2)]


def v_empty_chunk(n, grid, per):
    lo, hi = sr.chunks(n // 4, grid)[-1]
    assert lo > n // 4 and not any(per[grid - 1, t] for t in range(sr.VADD_WG))


def v_one_word_no_scalars(n, grid, per):
    assert [(k, dict(c)) for k, c in per.items() if c] == [((0, 0), {"vec": 1})]


def v_scalars_only(n, grid, per):
    assert n // 4 == 0 and [(k, dict(c)) for k, c in sorted(per.items()) if c] == [((0, t), {"scalar": 1}) for t in range(3)]


def v_single_item(n, grid, per):
    assert [(k, dict(c)) for k, c in per.items() if c] == [((0, 0), {"scalar": 1})]


def v_production(n, grid, per):
    assert grid == 28                                  # 7001 words rounded up to 256-lane workgroups


VADD_PROPERTIES = {f.__name__[2:]: f for f in (v_ten_ragged_iterations_three_scalars, v_one_wave_per_chunk_and_scalars,
                                              v_empty_chunk, v_one_word_no_scalars, v_scalars_only, v_single_item,
                                              v_production)}


@pytest.mark.parametrize("shape", sr.VADD_SHAPES, ids=sr.shape_id)
def test_vadd_shape_covers_its_range_and_has_its_property(shape):
    n, grid, prop = shape
    grid = sr.vadd_grid(n, grid)
    visits = sr.vadd_visits(n, grid)
    exactly_once(visits, n)
    VADD_PROPERTIES[prop](n, grid, iterations(visits, grid, sr.VADD_WG))
