#!/bin/bash
# PPO: its bench line with the roofline (--full) and rocprofv3 kernel stats of the bench command; results under $OUT
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$(mktemp -d)}; mkdir -p "$OUT"; echo "results: $OUT"
cd $R
timeout 300 python bench.py --full --algo ppo --steps 30 > $OUT/bench_ppo.json 2>/dev/null; python -c "import json;d=json.loads(open('$OUT/bench_ppo.json').read().strip().splitlines()[-1]);print('ppo', round(d['value']), d['ms_per_step'], d['learner_updates_per_s'], d['roofline']['frac'], d['roofline']['avg_launch_ms'], d['roofline']['share_of_iteration'])"
cd /tmp && export TMPDIR=/tmp && rm -rf /tmp/profp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/profp -- python $R/bench.py --algo ppo --steps 30 --no-cpu-baseline > /dev/null 2>&1
f=$(find /tmp/profp -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -20 "$f" > $OUT/ppo_kernel_stats.csv; head -6 $OUT/ppo_kernel_stats.csv | cut -c1-150
