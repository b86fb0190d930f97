#!/bin/bash
# A/B of a decode switch on one bench line: scripts/gpu_ab.sh ENVVAR [bench args]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${WSG_OUT:-bench_out}  # where the runs' JSON lines and stderr go
mkdir -p "$OUT"
var=$1; shift
for v in 1 0 1 0; do
  env $var=$v timeout -k 10 120 python bench.py --full --steps 20 --warmup 3 --no-extras --no-cpu-baseline --extra-steps 10 "$@" > "$OUT/ab.json" 2>"$OUT/ab.err" || { tail -5 "$OUT/ab.err"; exit 1; }
  python -c "import json;d=json.load(open('$OUT/ab.json'));print('$var=$v', d['value'], d['ms_per_step'], d['roofline']['avg_launch_ms'], d['pipeline_ms'])"
done
