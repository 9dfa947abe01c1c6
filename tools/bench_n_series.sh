#!/bin/bash
# SURVEY 8(d) scaling series on one GPU: the headline bench (--full: roofline, end_to_end) at N = 4k .. 100k (same
# generator, g=12 m=8, 495 combos). One JSON line per N into the file named by the first argument.
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${1:?usage: tools/bench_n_series.sh OUT.jsonl}
mkdir -p "$(dirname "$OUT")"; : > "$OUT"
for n in 4000 8000 16000 32000 64000 100000; do
  python3 "$R/bench.py" --full --n-seq $n --steps 3 --warmup 1 --no-cpu-baseline --no-also 2>/dev/null | grep '^{' >> "$OUT"
done
