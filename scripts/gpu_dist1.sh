#!/bin/bash
# bench.py in the launcher form at world size 1 over RCCL, with the --full extras (per-rank local rate -> multi_gpu.expected)
set -u
OUT="${OUT:-bench_out}"; mkdir -p "$OUT"; export TMPDIR=/tmp
R="${GRAFT_REPO_ROOT:-$PWD}"; cd "$R"
timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 4 --warmup 2 --full --no-cpu-baseline > "$OUT/bench_dist1.log" 2>&1
echo "rc=$?" >> "$OUT/bench_dist1.log"
grep -v "amdgpu.ids" "$OUT/bench_dist1.log" | tail -5 | cut -c1-900
