#!/bin/bash
# A/B of builds of libwsgpu.so on the same box, interleaved:
#   scripts/ab_lib.sh <lib_a.so> <lib_b.so> [<lib_c.so> ...] [bench args]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${WSG_OUT:-bench_out}  # where the runs' JSON lines and stderr go
mkdir -p "$OUT"
LIBS=()
while [[ "$1" == *.so ]]; do LIBS+=("$1"); shift; done
for round in 1 2 3; do for lib in "${LIBS[@]}"; do
  WSG_LIB=$lib timeout -k 10 120 python bench.py --full --steps 20 --warmup 3 --no-extras --no-cpu-baseline --extra-steps 10 "$@" > "$OUT/ab.json" 2>"$OUT/ab.err" || { tail -5 "$OUT/ab.err"; exit 1; }
  python -c "import json;d=json.load(open('$OUT/ab.json'));r=d['roofline'];print('$(basename $lib)', d['value'], d['ms_per_step'], r['avg_launch_ms'], r.get('frac_of_copy_ceiling'), d.get('pipeline_ms'))"
done; done
