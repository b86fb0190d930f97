#!/bin/bash
# A/B of libwsgpu.so builds on the PCIe-inclusive paths (bench.py --e2e), interleaved:
#   scripts/ab_e2e.sh <lib_a.so> <lib_b.so> [...]
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${WSG_OUT:-bench_out}  # where the runs' JSON lines and stderr go
mkdir -p "$OUT"
for round in 1 2 3; do for lib in "$@"; do
  WSG_LIB=$lib timeout -k 10 240 python bench.py --full --steps 3 --warmup 1 --no-extras --no-cpu-baseline --e2e > "$OUT/abe2e.json" 2>"$OUT/abe2e.err" || { tail -5 "$OUT/abe2e.err"; exit 1; }
  python -c "import json;d=json.load(open('$OUT/abe2e.json'))['e2e_pinned'];n=d['native_batcher'];print('$(basename $lib)', 'pipelined', d['pipelined']['GiB_per_s'], 'native', n['GiB_per_s'], 'feed', n['feed_GiB_per_s'])"
done; done
