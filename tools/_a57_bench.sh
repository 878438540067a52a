#!/bin/bash
# Agent57_light: its GPU tests, its bench line with the roofline (--full), rocprofv3 kernel stats of the bench command, graph-replay check; results under $OUT
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$(mktemp -d)}; mkdir -p "$OUT"; echo "results: $OUT"
cd $R
timeout 600 python -m pytest tests/test_agent57_fast_gpu.py tests/test_dist_gpu.py tests/test_dist_stream_semantics_gpu.py -x -q -m gpu 2>&1 | tail -2
timeout 500 python bench.py --full --algo agent57_light --envs 1024 --capacity 200000 --steps 4 --inner 16 --warmup 1 > $OUT/bench_agent57_light.json 2>/dev/null; python -c "import json;d=json.loads(open('$OUT/bench_agent57_light.json').read().strip().splitlines()[-1]);print('agent57_light', round(d['value']), d['ms_per_lock_step'], d['learner_updates_per_s'], d['roofline']['frac'])"
cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/profa
timeout 500 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/profa -- python $R/bench.py --algo agent57_light --envs 1024 --capacity 200000 --steps 4 --inner 16 --warmup 1 > /dev/null 2>&1
f=$(find /tmp/profa -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -40 "$f" > $OUT/a57_kernel_stats.csv
cd $R; python tools/graph_replay_check.py 2>&1 | grep "agent57_light: distinct"
