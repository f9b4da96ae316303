#!/bin/bash
# Measurement set: both GAME config-5 presets and the whole benchmark record (bench.py --full). Output under
# bench_results/.
set -o pipefail
out=bench_results
mkdir -p $out
export TMPDIR=/tmp
for cfg in game5 game5pl; do
  timeout -k 10 900 python -u bench_game.py --config $cfg --steps 3 --warmup 2 > $out/final_$cfg.json 2> $out/final_$cfg.log || { echo "bench $cfg failed"; tail -30 $out/final_$cfg.log; exit 1; }
  grep -E "built in|coordinate (global|per-entity)" $out/final_$cfg.log | tail -3
  cat $out/final_$cfg.json | cut -c1-240
done
timeout -k 10 900 python bench.py --full > $out/final_bench.json 2> $out/final_bench.log || { echo "bench failed"; tail -30 $out/final_bench.log; exit 1; }
cat $out/final_bench.json | cut -c1-240
