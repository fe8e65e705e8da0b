#!/bin/bash
# full GPU suite, then the full bench line (heads and tails of the solves reworked)
#   bash tools/check_all.sh OUT_DIR      (the test log and the bench line land in OUT_DIR)
set -e
out=${1:?usage: tools/check_all.sh OUT_DIR}
mkdir -p "$out"
python -m pytest tests -x -q -m gpu > "$out/r_tests.log" 2>&1 || { tail -40 "$out/r_tests.log"; exit 1; }
tail -3 "$out/r_tests.log"
python bench.py --full --steps 20 --warmup 5 > "$out/r_bench.json" 2> "$out/r_bench.err" || { tail -20 "$out/r_bench.err"; exit 1; }
python - "$out/r_bench.json" <<'PY'
import json
import sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k: d[k] for k in ('value', 'ms_per_step')}, d.get('breakdown_ms_per_step'))
for k in ('bundled_15k_pair', 'messy_250k_pair', 'c5_1m_k10'):
    v = d.get(k, {})
    print(k, v.get('ms'), v.get('breakdown_ms'))
PY
