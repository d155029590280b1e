#!/bin/bash
# One GPU run that refreshes the tracked round summaries: default bench line with every secondary figure (--full), bf16 /
# surface / cylinder lines, and the kernel trace of the default step (summarised by profiles/summarize.py).
#   bash profiles/round_profile.sh r02        (outputs under $PROFILE_OUT/r02, default profile_out/r02)
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
tag=${1:-rXX}
out=${PROFILE_OUT:-profile_out}/$tag
mkdir -p $out
timeout 600 python bench.py --full > $out/bench_default.json 2> $out/bench_default.err
timeout 300 python bench.py --full --dtype bf16 --no-cpu-baseline > $out/bench_bf16.json 2>/dev/null
timeout 300 python bench.py --full --workload surface --batch 2 --no-cpu-baseline > $out/bench_surface.json 2>/dev/null
timeout 300 python bench.py --full --workload surface --batch 2 --dtype bf16 --no-cpu-baseline > $out/bench_surface_bf16.json 2>/dev/null
timeout 300 python bench.py --full --dtype bf16_nodes --no-cpu-baseline > $out/bench_bf16_nodes.json 2>/dev/null
timeout 300 python bench.py --full --workload surface --batch 2 --dtype bf16_nodes --no-cpu-baseline > $out/bench_surface_bf16_nodes.json 2>/dev/null
timeout 300 python bench.py --full --workload cylinder --no-cpu-baseline > $out/bench_cyl.json 2>/dev/null
timeout 300 python bench.py --full --workload cylinder --layout blockdiag --no-cpu-baseline > $out/bench_cyl_blockdiag.json 2>/dev/null
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o r -- python bench.py --steps 10 --warmup 3 > $out/prof.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_bf16 -o r -- python bench.py --dtype bf16 --steps 10 --warmup 3 > $out/prof_bf16.log 2>&1
tail -n 1 $out/bench_*.json | cut -c1-400
