#!/bin/bash
# process-to-process variation of the bench step: 8 processes, each with its breakdown (their stderr goes to the log too)
set -e
mkdir -p gpurun_out
for i in 1 2 3 4 5 6 7 8; do
  python bench.py --steps 12 --warmup 4 --no-extras --no-cpu-baseline | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$i: %.3f ms' % d['ms_per_step'], {k: round(v,3) for k,v in d['breakdown_ms_per_step'].items()})"
done 2>&1 | tee gpurun_out/t_var.log
