#!/usr/bin/env bash
# tools/sweep_cube.sh -- light-cube resolution sweep (MIRT_CUBE_BINS) on the two soup workloads
o=$(mktemp)
for cb in 64 128 256; do
  MIRT_CUBE_BINS=$cb python bench.py --full --workload soup1m8k --no-cpu-baseline --steps 3 --warmup 1 2>/dev/null > "$o"
  python -c "import json, sys; d=json.load(open(sys.argv[1])); print('1M cube $cb', d['ms_per_step'], d['value'], d['kernel_ms_rank0'], d['roofline']['tests_per_launch'])" "$o"
done
for cb in 64 128; do
  MIRT_CUBE_BINS=$cb python bench.py --full --workload soup100k --no-cpu-baseline 2>/dev/null > "$o"
  python -c "import json, sys; d=json.load(open(sys.argv[1])); print('100k cube $cb', d['ms_per_step'], d['value'], d['kernel_ms_rank0'], d['roofline']['tests_per_launch'])" "$o"
done
rm -f "$o"
