"""In-process HIP validation kernels (amdkube._native._hipops, built from native/hipops.hip
and kernels/gpu_common.h for gfx950). Importing this module on a machine with /dev/kfd but
without the built extension raises — GPU code paths never fall back silently."""
from __future__ import annotations

import os

try:
    from .._native import _hipops as _ext  # type: ignore
except ImportError as e:
    _ext = None
    _err = e
    if os.path.exists("/dev/kfd") or os.environ.get("AMDKUBE_REQUIRE_NATIVE") == "1":
        raise ImportError(f"amdkube HIP extension _hipops not built (python native/build.py): {e}")


def _need():
    if _ext is None:
        raise RuntimeError(f"HIP extension unavailable: {_err}")
    return _ext


def device_count() -> int:
    return _need().device_count()


def device_info(device: int = 0) -> dict:
    return _need().device_info(device)


def vector_add(n: int = 50000, device: int = 0) -> dict:
    return _need().vector_add(n, device)


def hbm_probe(mib: int = 1024, iters: int = 5, device: int = 0) -> dict:
    return _need().hbm_probe(mib, iters, device)


def mfma_burn(ms: float = 100.0, device: int = 0) -> dict:
    return _need().mfma_burn(ms, device)


# ---- the same kernels on caller data (numerics checks against torch fp32 references) --------
def _np(x, dtype):
    import numpy as np
    if hasattr(x, "detach"):             # a torch tensor: host copy, contiguous
        x = x.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def vector_add_tensors(a, b, device: int = 0, grid: int = 0):
    """c = a + b with the pod workload's gfx950 vadd kernel; torch in → torch out. `grid` is the number
    of workgroups, 0 for the production grid."""
    import numpy as np
    import torch
    av, bv = _np(a, np.float32).ravel(), _np(b, np.float32).ravel()
    if av.shape != bv.shape:
        raise ValueError(f"shape mismatch {av.shape} vs {bv.shape}")
    return torch.from_numpy(np.asarray(_need().vector_add_arrays(av, bv, device, grid))).reshape(tuple(a.shape))


def mfma_tile(a, b, device: int = 0):
    """C = A @ B on one wave with v_mfma_f32_32x32x16_bf16: A is 32×K, B is K×32 (K a multiple of
    16); inputs are rounded to bf16 as the matrix core sees them, the result is fp32."""
    import numpy as np
    import torch
    a = torch.as_tensor(a).to(torch.bfloat16).contiguous()
    b = torch.as_tensor(b).to(torch.bfloat16).contiguous()
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != 32 or b.shape[1] != 32 or a.shape[1] != b.shape[0]:
        raise ValueError(f"need A 32xK and B Kx32, got {tuple(a.shape)} and {tuple(b.shape)}")
    k = a.shape[1]
    bits = lambda t: t.view(torch.int16).numpy().view(np.uint16).ravel()   # noqa: E731
    return torch.from_numpy(np.asarray(_need().mfma_tile(bits(a), bits(b), k, device)).copy())


def mfma_gemm(a, b, device: int = 0):
    """C = A @ B with the LDS-staged 64×64 MFMA tile kernel (one workgroup per tile of C): A is M×K,
    B is K×N, M and N multiples of 64, K a multiple of 16; inputs are rounded to bf16 as the
    matrix core sees them, the result is fp32."""
    import numpy as np
    import torch
    a = torch.as_tensor(a).to(torch.bfloat16).contiguous()
    b = torch.as_tensor(b).to(torch.bfloat16).contiguous()
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[0]:
        raise ValueError(f"need A MxK and B KxN, got {tuple(a.shape)} and {tuple(b.shape)}")
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    if m <= 0 or n <= 0 or m % 64 or n % 64 or k <= 0 or k % 16:
        raise ValueError(f"need M and N multiples of 64 and K a multiple of 16, got M={m} N={n} K={k}")
    bits = lambda t: t.view(torch.int16).numpy().view(np.uint16).ravel()   # noqa: E731
    return torch.from_numpy(np.asarray(_need().mfma_gemm(bits(a), bits(b), m, n, k, device)).copy())


LP_DTYPES = ("fp8", "mxfp8", "mxfp4")     # the low-precision matrix-core paths (kernels/mfma_check_lp.h)


def _codes(x, what):
    import numpy as np
    x = _np(x, None)
    if x.dtype != np.uint8 or x.ndim != 2:
        raise ValueError(f"{what} must be a 2-D uint8 array, got {x.dtype} {x.shape}")
    return x


def _gemm_lp(dtype, a, b, sa, sb, device):
    import numpy as np
    import torch
    m, k, n = a.shape[0], a.shape[1], b.shape[1]
    kstep = 16 if dtype == "fp8" else 64
    if b.shape[0] != k:
        raise ValueError(f"need A MxK and B KxN, got {a.shape} and {b.shape}")
    if m <= 0 or n <= 0 or m % 64 or n % 64 or k <= 0 or k % kstep:
        raise ValueError(f"need M and N multiples of 64 and K a multiple of {kstep}, got M={m} N={n} K={k}")
    if dtype == "fp8":
        sa = sb = np.zeros(0, np.uint8)
    elif sa.shape != (m, k // 32) or sb.shape != (k // 32, n):
        raise ValueError(f"need A scales Mx(K/32) and B scales (K/32)xN, got {sa.shape} and {sb.shape}")
    if dtype == "mxfp4" and (int(a.max()) > 15 or int(b.max()) > 15):
        raise ValueError("e2m1 codes must be in [0, 15]")
    c = _need().mfma_gemm_lp(dtype, a.ravel(), b.ravel(), sa.ravel(), sb.ravel(), m, n, k, device)
    return torch.from_numpy(np.asarray(c).copy())


def mfma_gemm_fp8(a, b, device: int = 0):
    """C = A @ B with the LDS-staged 64×64 tile kernel on v_mfma_f32_32x32x16_fp8_fp8: A is M×K, B is
    K×N, M and N multiples of 64, K a multiple of 16; inputs are rounded to OCP e4m3fn as the matrix
    core sees them, the result is fp32."""
    import torch
    from . import lowp
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f"need A MxK and B KxN, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _gemm_lp("fp8", lowp.encode_e4m3(a), lowp.encode_e4m3(b), None, None, device)


def mfma_gemm_mx(a_codes, a_scales, b_codes, b_scales, fmt: str, device: int = 0):
    """C = A @ B with the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 tile kernel. `fmt` is "fp8"
    (e4m3fn codes) or "fp4" (e2m1 codes, 0..15), one code per uint8; the E8M0 scales are uint8, A's as
    M×K/32 and B's as K/32×N (amdkube.ops.lowp.mx_quantize along K). M and N multiples of 64, K a
    multiple of 64; the result is an fp32 tensor."""
    if fmt not in ("fp8", "fp4"):
        raise ValueError(f"unknown MX element format {fmt!r}: expected fp8 or fp4")
    return _gemm_lp("mx" + fmt, _codes(a_codes, "A codes"), _codes(b_codes, "B codes"), _codes(a_scales, "A scales"),
                    _codes(b_scales, "B scales"), device)


def _check_dtype(dtype):
    if dtype != "bf16" and dtype not in LP_DTYPES:
        raise ValueError(f"unknown dtype {dtype!r}: expected bf16, {', '.join(LP_DTYPES)}")


def mfma_check(rounds: int | None = None, ms: float = 50.0, device: int = 0, seed: int = 0x5EED,
               selftest_flips: int = 0, dtype: str = "bf16") -> dict:
    """The matrix-core integrity check (mfma-check in process): every workgroup's MFMA product is
    compared with exact integer arithmetic in round 0 and bitwise with round 0 afterwards. `rounds`
    runs exactly that many, otherwise the run is calibrated to ~`ms`. `selftest_flips` perturbs
    that many compared values, which the check must then report. `dtype` picks the matrix-core path:
    bf16, fp8, mxfp8 or mxfp4; the result carries `dtype` and `tflops` (bf16 also `bf16_tflops`)."""
    _check_dtype(dtype)
    if rounds is not None and rounds < 1:
        raise ValueError("rounds must be at least 1")
    if dtype == "bf16":
        r = dict(_need().mfma_check(int(rounds or 0), float(ms), device, seed, selftest_flips))
        r["dtype"], r["tflops"] = "bf16", r["bf16_tflops"]
    else:
        r = dict(_need().mfma_check_lp(dtype, int(rounds or 0), float(ms), device, seed, selftest_flips))
    r["first_errors"] = [dict(e) for e in r["first_errors"]]
    return r


def mfma_check_tile(block: int, seed: int = 0x5EED, device: int = 0, dtype: str = "bf16"):
    """(A, B, C) of one workgroup of the check: its hashed 64×K and K×64 operands (decoded, with the
    block scales applied for the MX dtypes) and the 64×64 round-0 MFMA result, as fp32 tensors."""
    import numpy as np
    import torch
    _check_dtype(dtype)
    ext = _need()
    t = ext.mfma_check_tile(block, seed, device) if dtype == "bf16" else ext.mfma_check_lp_tile(dtype, block, seed, device)
    return tuple(torch.from_numpy(np.asarray(x).copy()) for x in t)


def cu_check(rounds: int | None = None, ms: float = 50.0, device: int = 0, seed: int = 0x5EED,
             selftest_flips: int = 0, units=("lds", "valu", "trans")) -> dict:
    """The per-CU integrity check (cu-check in process, kernels/cu_check.h): every workgroup owns a
    whole CU's LDS, marches all 160 KiB of it (`lds`), compares the same multiply-adds on the fp32,
    packed-fp32, fp64 and integer pipes (`valu`) and the transcendental unit on two waves (`trans`),
    and says where it ran. `rounds` runs exactly that many, otherwise the run is calibrated to ~`ms`.
    `selftest_flips` perturbs that many compared values, which the check must then report. The
    result carries the coverage (`cus`, `cus_covered`, `xccs`, `locations`, and `block_loc`, the raw
    location words of every workgroup of the timed launch), `errors_by_unit`, `bad_cus` and records
    with `unit`, `block`, `xcc`, `se`, `sh`, `cu`, `round`, `pass`, `index`, `got` and `want`. While
    places are missing, up to 3 further launches of one round are added (`launches`)."""
    from . import cucheck
    mask = cucheck.units_mask(units)
    if rounds is not None and rounds < 1:
        raise ValueError("rounds must be at least 1")
    if not 0 <= int(selftest_flips) <= cucheck.MAX_FLIPS:
        raise ValueError(f"selftest_flips must be in [0, {cucheck.MAX_FLIPS}]")
    r = dict(_need().cu_check(int(rounds or 0), float(ms), device, seed, int(selftest_flips), mask))
    for k in ("first_errors", "bad_cus", "locations"):
        r[k] = [dict(e) for e in r[k]]
    r["errors_by_unit"] = dict(r["errors_by_unit"])
    r["units"] = list(r["units"])
    return r


def cu_check_dump(block: int, seed: int = 0x5EED, device: int = 0) -> dict:
    """What workgroup `block` of a one-round check wrote and computed, as numpy arrays: `lds` (the
    40,960 words read back after pass 1), `valu_ops`, `valu_f32`, `valu_f64`, `valu_int`, `trans_in`,
    `trans_out` (layouts: amdkube.ops.cucheck), with the raw `hw_id` / `xcc_id` words and the decoded
    `location` of the workgroup."""
    import numpy as np
    from . import cucheck
    if block < 0:
        raise ValueError("block must not be negative")
    d = dict(_need().cu_check_dump(int(block), seed, device))
    for k, v in d.items():
        if k not in ("hw_id", "xcc_id"):
            d[k] = np.asarray(v).copy()
    d["location"] = cucheck.decode_location(d["hw_id"], d["xcc_id"])
    return d


def hbm_check(mib: int | None = None, rounds: int = 1, seed: int = 0x5EED, selftest_flips: int = 0, chunk_mib: int = 1024,
              hold_ms: int = 0, device: int = 0, free_fraction: float | None = None) -> dict:
    """The HBM integrity check (hbm-check in process, kernels/hbm_check.h): a march over `mib` MiB
    (default 1024), or over the share `free_fraction`, in (0, 0.95], of the device's free memory, in chunks
    of `chunk_mib` MiB. Each of `rounds` rounds writes an address-hashed background, reads it and writes
    its complement going up, reads that and writes the background going down, and reads it once more,
    every step over the whole region, with a host sleep of `hold_ms` between the second and the third.
    `selftest_flips` (at most 64) corrupts that many slots of the first chunk between those two steps of
    round 0, which the check must then report. The result carries `bytes`, `chunks` (bytes of each),
    `ms`, `alloc_ms`, `march_gbps`, `errors`, `bit_errors`, `transient`, `persistent`, `records_dropped`,
    `bad_pages` (`offset` in the region, `chunk`, `errors`; at most 32, with `bad_pages_total`) and
    `first_errors`: `round`, `pass`, `chunk`, `slot`, `word`, `got`, `want`, `again` and the `xcc`, `se`,
    `sh`, `cu` of the wave that read it."""
    from . import hbmcheck
    if mib is not None and free_fraction is not None:
        raise ValueError("give the region as mib or as free_fraction, not both")
    if mib is None and free_fraction is None:
        mib = 1024
    if mib is not None and int(mib) < 2:
        raise ValueError("mib must be at least 2 (one 2 MiB page)")
    if free_fraction is not None and not 0 < float(free_fraction) <= hbmcheck.FREE_FRACTION_MAX:
        raise ValueError("free_fraction must be in (0, 0.95]")
    if rounds < 1:
        raise ValueError("rounds must be at least 1")
    if not 0 <= int(selftest_flips) <= hbmcheck.RECORDS:
        raise ValueError(f"selftest_flips must be in [0, {hbmcheck.RECORDS}]")
    r = dict(_need().hbm_check(int(mib or 0), float(free_fraction or 0.0), int(chunk_mib), int(rounds), seed,
                               int(selftest_flips), int(hold_ms), device))
    r["chunks"] = [int(c) for c in r["chunks"]]
    for k in ("first_errors", "bad_pages"):
        r[k] = [dict(e) for e in r[k]]
    return r


def hbm_march_pass(words, seed: int, invert: bool, down: bool, write: bool, device: int = 0, grid: int = 0) -> dict:
    """One launch of the check's march kernel on `words` (uint32, four to a 16-byte slot): compare every
    word with the pattern of `seed`, complemented if `invert`, walking every workgroup's share downwards
    if `down`, and if `write` store the complement of what was expected. `grid` is the number of workgroups,
    0 for the production grid, as in the hbm_* wrappers below. Returns `words` after the pass,
    `errors`, `bit_errors`, `transient`, `persistent`, `records_dropped`, `page_errors` (one count per
    2 MiB) and `records` (at most 64, as `first_errors` of hbm_check)."""
    import numpy as np
    r = dict(_need().hbm_march_pass(_np(words, np.uint32).ravel(), seed, 0xFFFFFFFF if invert else 0, bool(down),
                                    bool(write), device, grid))
    r["words"], r["page_errors"] = np.asarray(r["words"]), np.asarray(r["page_errors"])
    r["records"] = [dict(e) for e in r["records"]]
    return r


# `grid` below is the number of workgroups to launch: 0 takes the production grid (sized from the CU
# count), anything else up to 65536 lets a test reach empty, ragged and unrolled-loop chunks at a few KiB.
def hbm_pattern(n16: int, seed: int = 0x5EED, device: int = 0, grid: int = 0):
    """The HBM probe's write pattern for n16 16-byte words, as uint32 words."""
    import numpy as np
    return np.asarray(_need().hbm_pattern(n16, seed, device, grid))


def hbm_verify(words, seed: int = 0x5EED, device: int = 0, grid: int = 0) -> int:
    """Mismatching 32-bit words of `words` against the probe pattern (the probe's verify kernel)."""
    import numpy as np
    return int(_need().hbm_verify_words(_np(words, np.uint32).ravel(), seed, device, grid))


def hbm_read(words, grid: int = 0, device: int = 0) -> int:
    """The probe's read kernel over `words`: it XORs every 32-bit word it loads, per lane, and a lane
    whose XOR is 0x9e3779b9 stores that value; returns what was stored, else 0."""
    import numpy as np
    return int(_need().hbm_read_words(_np(words, np.uint32).ravel(), grid, device))


def hbm_copy(words, device: int = 0, grid: int = 0):
    """`words` through the probe's copy kernel, into a destination that held 0xff bytes."""
    import numpy as np
    return np.asarray(_need().hbm_copy_words(_np(words, np.uint32).ravel(), device, grid))


# ---- hsa-vector-add's kernels (kernels/vadd_kernel.hip) from the code object that program embeds
VADD_CODE_OBJECT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_native", "lib", "vadd_gfx950.co")


def hsa_vadd_arrays(a, b, groups: int, device: int = 0):
    """c = a + b with `amdkube_vadd` on `groups` workgroups; float32 numpy in and out."""
    import numpy as np
    av, bv = _np(a, np.float32).ravel(), _np(b, np.float32).ravel()
    if av.shape != bv.shape:
        raise ValueError(f"shape mismatch {av.shape} vs {bv.shape}")
    return np.asarray(_need().hsa_vadd_arrays(VADD_CODE_OBJECT, av, bv, groups, device))


def hsa_copy_array(src, groups: int, device: int = 0):
    """`src` through `amdkube_copy` on `groups` workgroups; float32 numpy in and out, bit for bit."""
    import numpy as np
    return np.asarray(_need().hsa_copy_array(VADD_CODE_OBJECT, _np(src, np.float32).ravel(), groups, device))
