#!/bin/bash
# same-box A/B of one plan option: bash tools/ab_option.sh mlp_fused [reps]   -> gpurun_out/ab/ab_<option>.txt
opt=$1; reps=${2:-3}
mkdir -p gpurun_out/ab
F="--steps 50 --warmup 5 --windows 5 --full --no-cpu-baseline --profile-steps 0 --small-batch-steps 0 --fp32-steps 0 --f16x3-steps 0"
: > gpurun_out/ab/ab_$opt.txt
for rep in $(seq $reps); do
  for v in 0 1; do
    python bench.py $F --option $opt=$v 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$opt=$v value', d['value'], 'ms', d['ms_per_step'], 'launches', d['config']['launches_per_step'], 'sclk', d['sclk_mhz']['median_window']['median'])" | tee -a gpurun_out/ab/ab_$opt.txt
  done
done
