#!/bin/bash
# A/B of an environment switch on one build, interleaved:
#   scripts/ab_env.sh WSG_TUNE_<NAME> "v1 v2 ..." (bench.py apply_tuning) <python expr over d (the JSON line)> [bench args]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${WSG_OUT:-bench_out}  # where the runs' JSON lines and stderr go
mkdir -p "$OUT"
VAR=$1; VALS=$2; EXPR=$3; shift 3
for round in 1 2 3; do for v in $VALS; do
  env "$VAR=$v" timeout -k 10 150 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --extra-steps 10 "$@" > "$OUT/ab.json" 2>"$OUT/ab.err" || { tail -5 "$OUT/ab.err"; exit 1; }
  python -c "import json;d=json.load(open('$OUT/ab.json'));print('$VAR=$v', $EXPR)"
done; done
