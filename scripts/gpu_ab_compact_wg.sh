#!/bin/bash
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export TMPDIR=/tmp; out=${BENCH_OUT:-bench_out}; mkdir -p "$out"
for v in w1024 base w1024b baseb; do
  a=""; case $v in w1024*) a="--flag compact_wg=1024";; esac
  timeout -k 10 300 python -u bench.py --full --cpu-budget 0 $a > $out/h_$v.json 2> $out/h_$v.err || { tail -20 $out/h_$v.err; exit 1; }
  python3 -c "
import json;d=json.load(open('$out/h_$v.json'));print('$v', d['value'], d['ms_per_step'], d['roofline']['avg_launch_us'])"
done
