"""The host-side reference of the per-CU check (amdkube/ops/cucheck.py) and the argument checks of
hip.cu_check, which are made before the extension is called (CPU tier)."""
import numpy as np
import pytest

from amdkube.ops import cucheck, hip


def test_decode_location_takes_the_documented_fields_only():
    assert cucheck.decode_location(0, 0) == {"xcc": 0, "se": 0, "sh": 0, "cu": 0}
    hw = (5 << 13) | (1 << 12) | (9 << 8)
    assert cucheck.decode_location(hw, 6) == {"xcc": 6, "se": 5, "sh": 1, "cu": 9}
    # wave, SIMD, pipe, thread-group, VM, queue, state and ME bits are not part of a place
    noise = 0xFFFF00FF
    assert cucheck.decode_location(hw | noise, 6 | 0xFFFFFFF0) == cucheck.decode_location(hw, 6)
    for field, word in (("cu", 15 << 8), ("sh", 1 << 12), ("se", 7 << 13)):
        d = cucheck.decode_location(word, 0)
        assert d.pop(field) == word >> {"cu": 8, "sh": 12, "se": 13}[field] and set(d.values()) == {0}
    assert cucheck.decode_location(0, 15)["xcc"] == 15


def test_mix32_and_key_match_the_header_on_known_values():
    # mix32 of gpu_common.h, worked by hand in Python integers
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    for x in (0, 1, 0x5EED, 0xFFFFFFFF, 0x9E3779B9):
        assert int(cucheck.mix32(x)) == mix(x)
    seed, block, tag = 0x5EED, 1023, 0x4C000002
    assert int(cucheck.key(seed, block, tag)) == mix((mix(seed ^ (0x9E3779B9 * (block + 1)) & 0xFFFFFFFF) + tag) & 0xFFFFFFFF)


def test_lds_pattern_differs_between_rounds_and_blocks_and_pass_2_is_the_complement():
    p = cucheck.lds_pattern(0x5EED, 0, 0, 1)
    assert p.dtype == np.uint32 and p.shape == (40960,)
    assert len(np.unique(p)) == 40960                                  # a bijection of the word address
    for other in (cucheck.lds_pattern(0x5EED, 0, 1, 1), cucheck.lds_pattern(0x5EED, 1, 0, 1),
                  cucheck.lds_pattern(12345, 0, 0, 1)):
        assert (other != p).mean() > 0.99
    assert np.array_equal(cucheck.lds_pattern(0x5EED, 0, 0, 2), ~p)
    assert np.array_equal(cucheck.lds_pattern(0x5EED, 0, 0, 3), p)
    step = np.diff(p.astype(np.int64)) % 2 ** 32                       # P(wa) = wa * mul + add with an odd mul
    assert len(np.unique(step)) == 1 and step[0] % 2 == 1
    with pytest.raises(ValueError):
        cucheck.lds_pattern(0x5EED, 0, 0, 4)


def test_valu_operands_are_in_range_and_the_fp32_form_stays_exact():
    for block in (0, 1023):
        ops = cucheck.valu_operands(0x5EED, block)
        assert ops.dtype == np.uint32 and ops.shape == (1024, 12)
        for a, b, c in ((0, 1, 2), (3, 4, 5)):
            assert ops[:, a].max() < 2 ** 12 and ops[:, b].max() < 2 ** 11 and ops[:, c].max() < 2 ** 23
            assert ops[:, a].max() > 2 ** 11 and ops[:, c].max() > 2 ** 22            # the range is used
        assert ops[:, 6:9].max() < 2 ** 26 and (ops[:, 10] & 1).all()
        want = cucheck.valu_expected(ops)
        assert want.dtype == np.int64 and want.shape == (1024, 4)
        assert want[:, :2].max() < 2 ** 24 and want[:, 2].max() < 2 ** 53 and want[:, 3].max() < 2 ** 32
        assert np.array_equal(want[:, 0].astype(np.float32).astype(np.int64), want[:, 0])
    assert not np.array_equal(cucheck.valu_operands(0x5EED, 0), cucheck.valu_operands(0x5EED, 1))
    # the chain by hand on one lane
    o = [int(v) for v in cucheck.valu_operands(7, 3)[5]]
    x = o[9]
    for _ in range(16):
        x = (x * o[10] + o[11]) % 2 ** 32
    assert int(cucheck.valu_expected(cucheck.valu_operands(7, 3))[5, 3]) == x


def test_trans_inputs_are_normal_in_range_and_shared_by_a_wave_pair():
    x = cucheck.trans_inputs(0x5EED, 0)
    assert x.dtype == np.float32 and x.shape == (1024, 5, 4)
    assert x[:, 0].min() >= -20 and x[:, 0].max() < 20 and x[:, 0].min() < -19 and x[:, 0].max() > 19
    for f in (1, 2, 3, 4):
        assert x[:, f].min() >= 2.0 ** -20 and x[:, f].max() < 2.0 ** 20
    assert not ((x[:, 1] >= 0.5) & (x[:, 1] < 2)).any()               # log2 keeps off the binades next to 1
    assert ((x[:, 2] >= 0.5) & (x[:, 2] < 2)).any()
    lanes = x.reshape(16, 64, 5, 4)
    for w in range(0, 16, 2):
        assert np.array_equal(lanes[w], lanes[w + 1])
    assert not np.array_equal(lanes[0], lanes[2])
    assert np.isfinite(cucheck.trans_reference(x)).all()


def test_units_mask():
    assert cucheck.units_mask(("lds", "valu", "trans")) == 7 and cucheck.units_mask(("trans",)) == 4
    assert cucheck.units_mask("lds,trans") == 5
    for bad in (("foo",), (), ("lds", "lds"), "lds,,valu"):
        with pytest.raises(ValueError):
            cucheck.units_mask(bad)


def test_bad_arguments_raise_before_the_extension_is_called(monkeypatch):
    def boom():
        raise AssertionError("the extension was asked")
    monkeypatch.setattr(hip, "_need", boom)
    with pytest.raises(ValueError):
        hip.cu_check(units=("foo",))
    with pytest.raises(ValueError):
        hip.cu_check(selftest_flips=5000)
    with pytest.raises(ValueError):
        hip.cu_check(selftest_flips=-1)
    with pytest.raises(ValueError):
        hip.cu_check(rounds=0)
    with pytest.raises(ValueError):
        hip.cu_check(units=())
    with pytest.raises(ValueError):
        hip.cu_check_dump(-1)
