"""Native / GPU operations used by the control plane and the validation workloads.

  topology  — xGMI/NUMA GPU-subset selection (C++ `_topo`, Python reference)
  hip       — in-process HIP (gfx950) kernels: vector add, HBM probe, MFMA burn, the checked bf16 / FP8 / MXFP8 /
              MXFP4 matrix-core GEMMs and integrity checks (`_hipops`)
  lowp      — host side of the low-precision formats: e4m3fn / e2m1 codes, E8M0 scales, MX quantisation
"""
