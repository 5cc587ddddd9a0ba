"""What the streaming kernels (vector add, HBM write / verify / read / copy) are held to, on the CPU:
the numpy re-derivation of the HBM probe's pattern, a model of each kernel's index arithmetic, and the
shapes the GPU tests run with the property each one is there for. tests/test_gpu_stream_kernels.py runs
the shapes on the GPU; tests/test_stream_shapes.py checks on the CPU that each shape has its property."""
import functools

import numpy as np

# The constants of the kernels, here and nowhere else in the tests: kernels/gpu_common.h (HBM_*, the
# 256 of every __launch_bounds__ and launch, write_front_grid) and kernels/vadd_contract.h (VADD_*,
# stream_grid). tests/test_stream_shapes.py compares them with those headers.
BLOCK = 256                     # lanes per workgroup of the HBM kernels
VADD_WG = 256                   # ... and of the three vector-add / copy kernels
WAVE = 64
HBM_UNROLL = 8                  # verify, read, copy: 16-byte loads in flight per lane in the main loop
HBM_WRITE_UNROLL = 2            # write: stores per lane and main-loop iteration
HBM_BLOCKS_PER_CU = 32          # verify and read
HBM_COPY_BLOCKS_PER_CU = 128
VADD_BLOCKS_PER_CU = 64
READ_MAGIC = 0x9E3779B9         # the one value hbm_read_kernel stores

MI355X_CUS = 256                # what the CPU model takes for grid = 0; the GPU tests ask the device


# ---------------------------------------------------------------------------- the pattern
def mix32(x):
    x = x & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


@functools.lru_cache(maxsize=None)
def pattern(n16, seed):
    """pattern() of gpu_common.h for items 0..n16-1 as 4 * n16 uint32 words (uint64 arithmetic, masked).
    Computed once for each (n16, seed) and shared: read-only."""
    i = np.arange(n16, dtype=np.uint64)
    base = ((i * 4) & 0xFFFFFFFF) ^ seed ^ ((i >> 30) & 0xFFFFFFFF)
    want = np.stack([mix32(base + j) for j in range(4)], axis=1).ravel().astype(np.uint32)
    want.setflags(write=False)
    return want


# ---------------------------------------------------------------------------- grids
def stream_grid(items, cus, per_cu):
    """stream_grid of vadd_contract.h."""
    return min(max((items + 255) // 256, 1), (cus if cus > 0 else 256) * per_cu)


def write_front_grid(cus):
    return cus // 2 if cus > 1 else 1


def chunked_grid(n16, grid, cus=MI355X_CUS, per_cu=HBM_BLOCKS_PER_CU):
    """The workgroups the verify / read (per_cu 32) or copy (128) wrapper launches for `grid`."""
    return grid or stream_grid(n16, cus, per_cu)


def write_grid(grid, cus=MI355X_CUS):
    return grid or write_front_grid(cus)


def vadd_grid(n, grid, cus=MI355X_CUS):
    """vector_add_host rounds the 16-byte words up for the production grid."""
    return grid or stream_grid((n + 3) // 4, cus, VADD_BLOCKS_PER_CU)


# ---------------------------------------------------------------------------- index arithmetic
def chunk_of(n, grid, block):
    """chunk_of of gpu_common.h (and chunk of vadd_kernel.hip): [lo, hi) of workgroup `block`. An empty
    chunk has hi <= lo, and lo may lie past n."""
    per = (n + grid - 1) // grid
    lo = block * per
    return lo, min(lo + per, n)


def chunks(n, grid):
    return [chunk_of(n, grid, b) for b in range(grid)]


def chunked_visits(n16, grid):
    """Every load of hbm_verify_kernel / hbm_read_kernel / hbm_copy_kernel launched on `grid` workgroups:
    (item, workgroup, lane, "main" or "tail", iteration of that loop)."""
    out = []
    for blk in range(grid):
        lo, hi = chunk_of(n16, grid, blk)
        for t in range(BLOCK):
            i, it = lo + t, 0
            while i + (HBM_UNROLL - 1) * BLOCK < hi:
                out += [(i + u * BLOCK, blk, t, "main", it) for u in range(HBM_UNROLL)]
                i += HBM_UNROLL * BLOCK
                it += 1
            it = 0
            while i < hi:
                out.append((i, blk, t, "tail", it))
                i += BLOCK
                it += 1
    return out


def write_visits(n16, grid):
    """Every store of hbm_write_kernel, as chunked_visits: a grid-stride front of grid * 256 lanes."""
    out = []
    st = grid * BLOCK
    for blk in range(grid):
        for t in range(BLOCK):
            i, it = blk * BLOCK + t, 0
            while i + (HBM_WRITE_UNROLL - 1) * st < n16:
                out += [(i + u * st, blk, t, "main", it) for u in range(HBM_WRITE_UNROLL)]
                i += HBM_WRITE_UNROLL * st
                it += 1
            it = 0
            while i < n16:
                out.append((i, blk, t, "tail", it))
                i += st
                it += 1
    return out


def vadd_visits(n, grid):
    """Every float vadd_kernel, amdkube_vadd and amdkube_copy touch: (float index, workgroup, lane,
    "vec" or "scalar", iteration). Chunks of 16-byte words, then the < 4 trailing floats in workgroup 0."""
    out = []
    n4 = n // 4
    for blk in range(grid):
        lo, hi = chunk_of(n4, grid, blk)
        for t in range(VADD_WG):
            for it, i in enumerate(range(lo + t, hi, VADD_WG)):
                out += [(4 * i + j, blk, t, "vec", it) for j in range(4)]
            if blk == 0:
                out += [(k, blk, t, "scalar", it) for it, k in enumerate(range(4 * n4 + t, n, VADD_WG))]
    return out


# ---------------------------------------------------------------------------- the shapes
# (n16, grid, property); grid 0 is the production grid. The properties are the predicates of
# tests/test_stream_shapes.py.
CHUNKED_SHAPES = [
    (7000, 3, "one_main_full_tail_partial_tail"),   # chunks 2334, 2334, 2332
    (3800, 2, "main_loop_splits_a_wave"),           # chunks of 1900: lanes < 108 take the main loop
    (2048, 1, "main_only"),
    (2049, 1, "main_plus_one_lane_tail"),
    (5, 4, "empty_chunk"),                          # per = 2, the fourth workgroup has lo = 6 > n16
    (1, 1, "single_item"),
    (65541, 0, "production_tail_only"),             # 257 workgroups of 256 items: what the suite ran before
]
WRITE_SHAPES = [
    (1337, 2, "one_main_partial_tail"),
    (900, 2, "main_loop_splits_a_wave"),            # global lanes < 388 take the main loop
    (512, 1, "main_only"),
    (513, 1, "main_plus_one_lane_tail"),
    (5, 4, "most_lanes_idle"),
    (1, 1, "single_item"),
    (65541, 0, "production"),
]
# (n floats, grid, property); the production grid goes to the HIP wrapper only, the code-object kernels
# always get a number of groups
VADD_SHAPES = [
    (28003, 3, "ten_ragged_iterations_three_scalars"),   # n4 = 7000
    (1027, 4, "one_wave_per_chunk_and_scalars"),
    (23, 4, "empty_chunk"),
    (4, 1, "one_word_no_scalars"),
    (3, 1, "scalars_only"),
    (1, 1, "single_item"),
    (28003, 0, "production"),
]


def shape_id(shape):
    return f"{shape[0]}x{shape[1]}"


def edge_items(n16, grid):
    """The items of a chunked shape where a wrong loop bound would show: the first and last of every
    chunk, items 107 and 108 of each 1900-item chunk (the last lane in the main loop and the first one
    out of it), and items 2047 and 2048 (the end of a whole main iteration) where they exist."""
    items = set()
    for lo, hi in chunks(n16, grid):
        if lo < hi:
            items |= {lo, hi - 1}
            if hi - lo == 1900:
                items |= {lo + 107, lo + 108}
    items |= {i for i in (2047, 2048) if i < n16}
    return sorted(items)
