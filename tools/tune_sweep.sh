#!/bin/bash
# one tuning key over several values, alternating on one box, three rounds:   tools/tune_sweep.sh <key> <v1> <v2> ... [-- bench args]
key=$1; shift
vals=(); while [ $# -gt 0 ] && [ "$1" != "--" ]; do vals+=("$1"); shift; done; [ "$1" = "--" ] && shift
for rep in 1 2 3; do for v in "${vals[@]}"; do
  python bench.py --full --no-cpu-baseline --no-streamed --no-cli-e2e --steps 100 --warmup 5 --reps 5 --tune $key=$v "$@" > /tmp/x.json 2>/tmp/x.err || { echo "$key=$v FAILED"; tail -3 /tmp/x.err; continue; }
  python -c "
import json; d=json.load(open('/tmp/x.json')); r=d['roofline']; print('$key=$v:', d['value'], 'fps | ms/step', d['ms_per_step'], 'steady', d['steady_ms_per_step'], 'drain', d['drain_ms'], '| kernel (events)', r['ms_per_launch'], 'alone', r['ms_per_launch_alone'], '| checked', d.get('results_checked'))"
done; done
