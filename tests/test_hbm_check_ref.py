"""The numpy reference of the HBM check (amdkube/ops/hbmcheck.py) on the CPU: what the GPU tests of
tests/test_gpu_hbm_check.py hold the march kernel against must itself be a MATS++ march. A memory with a
stuck bit is modelled here by forcing the bit after every pass."""
import collections

import numpy as np
import pytest

from amdkube.ops import hbmcheck as hc
from tests import stream_ref as sr
from tests.test_stream_shapes import CHUNKED_PROPERTIES, exactly_once, iterations

SEED = 0x5EED
# one round after E0: (pass, invert, down, write)
ELEMENTS = [(1, False, False, True), (2, True, True, True), (3, False, True, False)]


def test_the_pattern_is_the_probes():
    for n16, seed in ((1, 0), (7000, SEED), (65541, 0xC0FFEE11)):
        assert np.array_equal(hc.pattern(n16, seed), sr.pattern(n16, seed))
    assert hc.mix32(1) == 0x688990C0 and hc.mix32(0) == 0
    assert int(hc.mix32(np.array([1], np.uint64))[0]) == 0x688990C0
    assert hc.chunk_seed(SEED, 0, 0) == hc.mix32(hc.mix32(SEED ^ 0x9E3779B9))
    assert len({hc.chunk_seed(SEED, r, c) for r in range(8) for c in range(64)}) == 512
    assert (hc.BLOCK, hc.UNROLL) == (sr.BLOCK, sr.HBM_UNROLL)


def test_four_passes_over_a_clean_buffer_end_with_the_pattern_and_no_error():
    n16 = 7000
    words = hc.pattern(n16, SEED)                                   # E0
    for _, invert, down, write in ELEMENTS:
        r = hc.march_pass(words, SEED, invert, down, write)
        assert (r["errors"], r["bit_errors"], r["transient"], r["persistent"]) == (0, 0, 0, 0)
        assert r["records"] == set() and r["page_errors"].tolist() == [0]
        words = r["words"]
    assert np.array_equal(words, hc.pattern(n16, SEED))
    after_e1 = hc.march_pass(hc.pattern(n16, SEED), SEED, False, False, True)["words"]
    assert np.array_equal(after_e1, ~hc.pattern(n16, SEED))


@pytest.mark.parametrize("stuck_at", [0, 1])
def test_a_stuck_bit_shows_in_the_passes_its_polarity_predicts_and_only_there(stuck_at):
    """A cell stuck at the value the background wants is wrong while the complement is stored: E2 alone
    reads it wrong. Stuck at the other value it is wrong under the background: E1 and E3."""
    n16, k, bit = 3800, 4 * 1907 + 2, 13
    mask = np.uint32(1 << bit)

    def memory(words):                                              # what the faulty part holds afterwards
        words = words.copy()
        words[k] = words[k] | mask if stuck_at else words[k] & ~mask
        return words

    background = (int(hc.pattern(n16, SEED)[k]) >> bit) & 1
    words = memory(hc.pattern(n16, SEED))
    seen = {}
    for pass_, invert, down, write in ELEMENTS:
        r = hc.march_pass(words, SEED, invert, down, write)
        seen[pass_] = r["errors"]
        if r["errors"]:
            (slot, word, got, want, again), = r["records"]
            assert (slot, word, got ^ want, again) == (1907, 2, 1 << bit, got)
            assert r["bit_errors"] == 1 and r["persistent"] == 1 and r["page_errors"].tolist() == [1]
        words = memory(r["words"])
    assert seen == ({1: 0, 2: 1, 3: 0} if background == stuck_at else {1: 1, 2: 0, 3: 1})


def test_the_output_complements_the_expected_value_not_the_read_one():
    n16 = 2049
    words = hc.pattern(n16, SEED).copy()
    words[4 * 2048 + 1] ^= np.uint32(0x00F00001)                    # five wrong bits in one word
    words[0:4] ^= np.uint32(1)                                      # all four words of slot 0
    r = hc.march_pass(words, SEED, False, False, True)
    assert np.array_equal(r["words"], ~hc.pattern(n16, SEED))       # the fault is not carried on
    assert (r["errors"], r["bit_errors"], r["persistent"], r["transient"]) == (5, 9, 5, 0)
    assert {(s, w) for s, w, *_ in r["records"]} == {(0, 0), (0, 1), (0, 2), (0, 3), (2048, 1)}
    assert hc.march_pass(r["words"], SEED, True, True, True)["errors"] == 0
    # without the write the buffer is what it was, and inverted expectations see every word wrong
    assert np.array_equal(hc.march_pass(words, SEED, False, True, False)["words"], words)
    assert hc.march_pass(hc.pattern(n16, SEED), SEED, True, False, False)["errors"] == 4 * n16


def test_page_errors_are_counted_per_2_mib():
    n16 = 2 * hc.PAGE_SLOTS + 5
    words = hc.pattern(n16, SEED).copy()
    for slot in (0, hc.PAGE_SLOTS - 1, hc.PAGE_SLOTS, 2 * hc.PAGE_SLOTS + 4):
        words[4 * slot] ^= np.uint32(1 << 31)
    r = hc.march_pass(words, SEED, False, False, False)
    assert r["page_errors"].tolist() == [2, 1, 1] and r["errors"] == 4
    assert [hc.page_of(s) for s in (0, hc.PAGE_SLOTS - 1, hc.PAGE_SLOTS)] == [0, 0, 1]


@pytest.mark.parametrize("shape", sr.CHUNKED_SHAPES, ids=sr.shape_id)
@pytest.mark.parametrize("down", [False, True], ids=["up", "down"])
def test_the_walk_covers_each_shape_once_and_has_its_property(shape, down):
    """The downward walk splits main loop and tail over the distance from the top of a workgroup's share,
    so a shape keeps the property it was chosen for; the upward walk is the one of the copy kernel."""
    n16, grid, prop = shape
    grid = sr.chunked_grid(n16, grid, per_cu=sr.HBM_COPY_BLOCKS_PER_CU)
    visits = hc.march_visits(n16, grid, down)
    exactly_once(visits, n16)
    CHUNKED_PROPERTIES[prop](n16, grid, iterations(visits, grid, sr.BLOCK))
    if not down:
        assert visits == sr.chunked_visits(n16, grid)
    else:
        # lane t of a workgroup starts at the top slot of its share and every lane goes downwards
        first = {}
        order = collections.defaultdict(list)
        for slot, blk, t, _, _ in visits:
            first.setdefault((blk, t), slot)
            order[blk, t].append(slot)
        for (blk, t), slot in first.items():
            assert slot == sr.chunk_of(n16, grid, blk)[1] - 1 - t
        assert all(s == sorted(s, reverse=True) for s in order.values())


def test_flip_slots_are_distinct_for_every_count_up_to_64():
    n16 = 1 << 17
    for seed in (SEED, 0xC0FFEE11, 0, 0xFFFFFFFF):
        for n in range(65):
            slots = hc.flip_slots(seed, n, n16)
            assert len(slots) == n == len(set(slots)) and all(0 <= s < n16 for s in slots)
        assert hc.flip_slots(seed, 64, n16)[:7] == hc.flip_slots(seed, 7, n16)
        bits = [hc.flip_bit(seed, f) for f in range(64)]
        assert all(0 <= w < 4 and 0 <= b < 32 for w, b in bits) and len(set(bits)) > 16
    # the arithmetic of check_core.h's flip_positions, by hand for one seed
    base, stride = SEED * 2654435761 + 0x5BD1E995, (((SEED ^ 0x9E3779B9) * 0x85EBCA6B) % n16) | 1
    assert stride % 2 == 1 and hc.flip_slots(SEED, 3, n16) == [(base + i * stride) % n16 for i in range(3)]
