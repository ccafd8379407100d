#!/bin/bash
# cfg 3 bench line (with its CPU baseline) and rocprofv3 evidence at HEAD
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 300 python -u bench.py --full --config 3 > $OUT/bench_cfg3.log 2>&1 || { tail -5 $OUT/bench_cfg3.log; exit 1; }
grep '^{' $OUT/bench_cfg3.log | tail -1 > $OUT/bench_cfg3.json
python -c "
import json; d=json.load(open('$OUT/bench_cfg3.json')); print('cfg3', '%.4g'%d['value'], d['roofline']['kernel_avg_ms'], d['cpu_baseline']['value'])"
ROUND=r03_cfg3_s0 BENCH_ARGS="--config 3" bash scripts/profile.sh > $OUT/profile_cfg3_s0.log 2>&1 && echo profiled
