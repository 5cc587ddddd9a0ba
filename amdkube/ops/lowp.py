"""Low-precision number formats of the CDNA4 matrix cores, on the host: OCP e4m3fn (FP8), e2m1 (FP4)
and E8M0 block scales, with MX quantisation (one scale per 32 elements). Pure numpy / torch and
importable without a GPU; `amdkube.ops.hip.mfma_gemm_fp8` / `mfma_gemm_mx` take the codes these
helpers produce, and the GPU tests decode with them for their float64 references.

Codes are uint8 arrays, one code per byte (e2m1 codes are 0..15: sign in bit 3, then two exponent
bits and one mantissa bit). Encoding rounds to nearest even and saturates at the format's largest
finite value; NaN is refused for e2m1, which has none.
"""
from __future__ import annotations

import numpy as np

MX_BLOCK = 32
# the eight magnitudes of e2m1, by code & 7
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E2M1_MAX = 6.0
E4M3_MAX = 448.0
_E2M1 = np.array(E2M1_VALUES, dtype=np.float32)
_E2M1_MID = (_E2M1[:-1] + _E2M1[1:]) / 2          # a tie at midpoint i goes to the even code of i, i + 1
_FORMATS = {"fp8": E4M3_MAX, "fp4": E2M1_MAX}


def _f32(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().float().numpy()
    return np.asarray(x, dtype=np.float32)


def _u8(x, what):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.dtype != np.uint8:
        raise ValueError(f"{what} must be uint8, got {x.dtype}")
    return x


def encode_e2m1(x):
    """float → e2m1 codes (uint8, 0..15): round to nearest even, saturating at ±6."""
    x = _f32(x)
    if np.isnan(x).any():
        raise ValueError("e2m1 has no NaN")
    mag = np.abs(x)[..., None]
    idx = (mag > _E2M1_MID).sum(-1) + ((mag == _E2M1_MID) & (np.arange(7) % 2 == 1)).sum(-1)
    return (idx | (np.signbit(x) << 3)).astype(np.uint8)


def decode_e2m1(codes):
    """e2m1 codes → float32."""
    codes = _u8(codes, "e2m1 codes")
    if codes.size and int(codes.max()) > 15:
        raise ValueError("e2m1 codes must be in [0, 15]")
    return np.where(codes & 8, -_E2M1[codes & 7], _E2M1[codes & 7]).astype(np.float32)


def encode_e4m3(x):
    """float → OCP e4m3fn codes (uint8), torch's round-to-nearest-even conversion, saturating at ±448."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(_f32(x))).clamp(-E4M3_MAX, E4M3_MAX)      # NaN stays NaN
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def decode_e4m3(codes):
    """OCP e4m3fn codes → float32 (0x7f and 0xff are NaN)."""
    import torch
    codes = np.ascontiguousarray(_u8(codes, "e4m3 codes"))
    return torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()


def e8m0(exp):
    """Exponent(s) → E8M0 scale byte(s): 2^exp is byte exp + 127, exp in [-127, 127]."""
    e = np.asarray(exp)
    if not np.issubdtype(e.dtype, np.integer):
        raise ValueError("E8M0 exponents are integers")
    if e.size and (int(e.min()) < -127 or int(e.max()) > 127):
        raise ValueError("E8M0 exponents must be in [-127, 127]")
    return (e + 127).astype(np.uint8)


def decode_e8m0(scales):
    """E8M0 bytes → float32 powers of two (255 is NaN)."""
    scales = _u8(scales, "E8M0 scales")
    out = np.ldexp(np.float64(1.0), np.minimum(scales, 254).astype(np.int32) - 127).astype(np.float32)
    return np.where(scales == 255, np.float32(np.nan), out)


def _fmt(fmt):
    if fmt not in _FORMATS:
        raise ValueError(f"unknown MX element format {fmt!r}: expected fp8 or fp4")
    return (encode_e4m3, decode_e4m3) if fmt == "fp8" else (encode_e2m1, decode_e2m1)


def _blocks(a, axis):
    """a with `axis` moved last and split into (blocks, 32)."""
    a = np.moveaxis(a, axis, -1)
    if a.shape[-1] % MX_BLOCK:
        raise ValueError(f"the quantised axis must be a multiple of {MX_BLOCK}, got {a.shape[-1]}")
    return a.reshape(*a.shape[:-1], a.shape[-1] // MX_BLOCK, MX_BLOCK)


def mx_quantize(x, fmt: str, axis: int = -1):
    """MX quantisation along `axis`: (codes, scales), codes shaped like x and one E8M0 scale per 32
    elements (the axis shrinks by 32). The scale of a block is the smallest power of two under which
    its largest magnitude fits the element format, so data that is already representable (element
    values times a power of two per block) comes back exactly; an all-zero block gets scale 1."""
    encode, _ = _fmt(fmt)
    x = _f32(x)
    if not np.isfinite(x).all():
        raise ValueError("mx_quantize needs finite values")
    b = _blocks(x, axis)
    m, ex = np.frexp(b.astype(np.float64).__abs__().max(-1) / _FORMATS[fmt])     # amax / fmax = m 2^ex, m in [0.5, 1)
    e = np.where(m == 0, 0, np.where(m == 0.5, ex - 1, ex)).clip(-127, 127).astype(np.int32)
    codes = encode(b / np.ldexp(np.float64(1.0), e)[..., None])
    codes = np.moveaxis(codes.reshape(*b.shape[:-2], -1), -1, axis)
    return np.ascontiguousarray(codes), np.ascontiguousarray(np.moveaxis(e8m0(e), -1, axis))


def mx_dequantize(codes, scales, fmt: str, axis: int = -1):
    """(codes, scales) of mx_quantize → float32."""
    _, decode = _fmt(fmt)
    v = _blocks(decode(codes), axis)
    s = np.moveaxis(decode_e8m0(scales), axis, -1)
    if s.shape != v.shape[:-1]:
        raise ValueError(f"scales {np.shape(scales)} do not match codes {np.shape(codes)} along axis {axis}")
    out = (v.astype(np.float64) * s[..., None].astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(np.moveaxis(out.reshape(*v.shape[:-2], -1), -1, axis))
