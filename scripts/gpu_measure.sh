#!/bin/bash
# Measurement set: the whole benchmark record (bench.py --full) and GAME config 5 (uniform and power-law entity
# sizes), no profiler. Output under bench_results/.
set -o pipefail
out=bench_results
mkdir -p $out
export TMPDIR=/tmp
tag=${1:-latest}
timeout -k 10 600 python bench.py --full > $out/bench_$tag.json 2> $out/bench_$tag.log || { echo "bench failed"; tail -30 $out/bench_$tag.log; exit 1; }
cut -c1-200 $out/bench_$tag.json
for cfg in game5 game5pl; do
  timeout -k 10 900 python -u bench_game.py --config $cfg --steps 3 --warmup 2 > $out/${cfg}_$tag.json 2> $out/${cfg}_$tag.log || { echo "bench $cfg failed"; tail -30 $out/${cfg}_$tag.log; exit 1; }
  grep -E "coordinate (global|per-entity)" $out/${cfg}_$tag.log | tail -2
  cut -c1-200 $out/${cfg}_$tag.json
done
