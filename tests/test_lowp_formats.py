"""amdkube.ops.lowp: the host side of the low-precision matrix-core formats: e2m1 and e4m3fn codes,
E8M0 scales and MX quantisation with one scale per 32 elements (CPU tier)."""
import numpy as np
import pytest

from amdkube.ops import lowp


def test_e2m1_round_trips_all_16_codes():
    codes = np.arange(16, dtype=np.uint8)
    v = lowp.decode_e2m1(codes)
    assert v.dtype == np.float32
    assert list(v[:8]) == list(lowp.E2M1_VALUES) == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert list(v[8:]) == [-x for x in lowp.E2M1_VALUES] and np.signbit(v[8])                 # code 8 is -0
    assert np.array_equal(lowp.encode_e2m1(v), codes)
    with pytest.raises(ValueError):
        lowp.decode_e2m1(np.array([16], np.uint8))
    with pytest.raises(ValueError):
        lowp.decode_e2m1(np.array([1.0], np.float32))


def test_e2m1_rounds_to_nearest_even_and_saturates():
    # every midpoint between neighbours goes to the one with an even mantissa bit (an even code)
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    for x, want in ties.items():
        assert float(lowp.decode_e2m1(lowp.encode_e2m1([x]))[0]) == want, x
        assert float(lowp.decode_e2m1(lowp.encode_e2m1([-x]))[0]) == -want, x
    near = {0.2: 0.0, 0.3: 0.5, 1.2: 1.0, 1.3: 1.5, 2.4: 2.0, 2.6: 3.0, 4.9: 4.0, 5.1: 6.0}
    for x, want in near.items():
        assert float(lowp.decode_e2m1(lowp.encode_e2m1([x]))[0]) == want, x
    assert list(lowp.decode_e2m1(lowp.encode_e2m1([7.0, 100.0, np.inf, -6.5, -1e30, -np.inf]))) == [6, 6, 6, -6, -6, -6]
    with pytest.raises(ValueError):
        lowp.encode_e2m1([np.nan])


def test_e4m3_helpers_agree_with_torch_on_all_256_codes():
    import torch
    codes = np.arange(256, dtype=np.uint8)
    v = lowp.decode_e4m3(codes)
    t = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    nan = np.isnan(t)
    assert list(codes[nan]) == [0x7F, 0xFF] and np.array_equal(np.isnan(v), nan)
    assert np.array_equal(v[~nan], t[~nan]) and float(np.abs(v[~nan]).max()) == lowp.E4M3_MAX == 448.0
    assert np.array_equal(lowp.encode_e4m3(v[~nan]), codes[~nan])
    # between codes: torch's rounding; beyond the range: saturation
    x = np.linspace(-500, 500, 4001, dtype=np.float32)
    want = torch.from_numpy(x).clamp(-448, 448).to(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(lowp.decode_e4m3(lowp.encode_e4m3(x)), want)
    assert list(lowp.decode_e4m3(lowp.encode_e4m3([1e6, -1e6]))) == [448.0, -448.0]
    assert lowp.encode_e4m3(torch.tensor([1.0, -2.0])).tolist() == [0x38, 0xC0]               # torch in, too


def test_e8m0():
    assert lowp.e8m0(np.array([-127, -1, 0, 1, 127])).tolist() == [0, 126, 127, 128, 254]
    assert lowp.decode_e8m0(np.array([126, 127, 128, 130], np.uint8)).tolist() == [0.5, 1.0, 2.0, 8.0]
    assert np.isnan(lowp.decode_e8m0(np.array([255], np.uint8))[0])
    for bad in ([128], [-128]):
        with pytest.raises(ValueError):
            lowp.e8m0(np.array(bad))
    with pytest.raises(ValueError):
        lowp.e8m0(np.array([0.5]))


@pytest.mark.parametrize("fmt,ncodes", [("fp8", 256), ("fp4", 16)])
@pytest.mark.parametrize("axis", [0, 1])
def test_mx_round_trip_is_exact_for_representable_data(fmt, ncodes, axis):
    rng = np.random.default_rng(ncodes + axis)
    shape = (96, 64) if axis == 0 else (64, 96)
    codes = rng.integers(0, ncodes, shape).astype(np.uint8)
    if fmt == "fp8":
        codes[(codes & 0x7F) == 0x7F] = 0x7E                          # no NaN codes
    sshape = (3, 64) if axis == 0 else (64, 3)
    scales = lowp.e8m0(rng.integers(-6, 7, sshape))
    x = lowp.mx_dequantize(codes, scales, fmt, axis)
    assert x.shape == shape and x.dtype == np.float32
    q, s = lowp.mx_quantize(x, fmt, axis)
    assert q.shape == shape and q.dtype == np.uint8 and s.shape == sshape and s.dtype == np.uint8
    assert np.array_equal(lowp.mx_dequantize(q, s, fmt, axis), x)


@pytest.mark.parametrize("fmt,fmax", [("fp8", 448.0), ("fp4", 6.0)])
def test_mx_quantize_picks_one_scale_per_32_elements_along_either_axis(fmt, fmax):
    # block b of every row holds magnitudes up to fmax * 2^(b - 2): its scale must be 2^(b - 2)
    base = np.linspace(-fmax, fmax, 32, dtype=np.float32)
    x = np.concatenate([base * 2.0 ** (b - 2) for b in range(4)])[None, :].repeat(5, 0)      # 5 x 128
    x[3, 32:64] = 0                                                                          # an all-zero block
    q, s = lowp.mx_quantize(x, fmt, axis=1)
    want = np.array([[125, 126, 127, 128]] * 5, np.uint8)
    want[3, 1] = 127
    assert np.array_equal(s, want)
    qt, st = lowp.mx_quantize(x.T.copy(), fmt, axis=0)
    assert np.array_equal(st, want.T) and np.array_equal(qt, q.T)
    # within a block the elements share the scale: the largest magnitude is the format's largest value
    d = lowp.mx_dequantize(q, s, fmt, axis=1)
    assert float(np.abs(d[0, :32]).max()) == fmax / 4 and float(np.abs(d[0, 96:]).max()) == fmax * 2
    # an error of at most half a step of the top binade, relative to the block's largest magnitude
    assert float(np.abs(d - x).max() / np.abs(x).max()) <= (2.0 ** -4 if fmt == "fp8" else 2.0 ** -2)


def test_mx_helpers_refuse_bad_arguments():
    x = np.zeros((4, 48), np.float32)
    with pytest.raises(ValueError):
        lowp.mx_quantize(x, "fp8", axis=1)                            # 48 is not a multiple of 32
    with pytest.raises(ValueError):
        lowp.mx_quantize(np.zeros((4, 64), np.float32), "fp6", axis=1)
    with pytest.raises(ValueError):
        lowp.mx_quantize(np.full((4, 64), np.inf, np.float32), "fp4", axis=1)
    with pytest.raises(ValueError):
        lowp.mx_dequantize(np.zeros((4, 64), np.uint8), np.zeros((4, 3), np.uint8), "fp4", axis=1)
