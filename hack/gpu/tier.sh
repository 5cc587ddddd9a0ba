#!/bin/bash
# GPU evidence pass: GPU test tier, smoke, 1-GPU bench with its extras (GPU pods + node density +
# scheduler_perf + hollow-node density). Logs go to $OUT (default gpu_out/).
set -e
OUT=${OUT:-gpu_out}
mkdir -p "$OUT"
timeout -k 10 600 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
timeout -k 10 900 python bench.py --full --steps 20 --warmup 2 > "$OUT/bench_n1.log" 2>&1
echo done
