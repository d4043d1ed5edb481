#!/bin/bash
# Final-state profiles of the default bench command (run on the GPU box through gpurun):
#   rocprofv3 --kernel-trace --stats of `python bench.py --full`, summarised into $OUT_DIR (default profile_out/) for copying
#   into profiles/.
# Usage: bash tools/profile_bench.sh <tag>      (counters are collected separately: tools/pmc_passes.sh)
set -u
tag=${1:-r01_final}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${OUT_DIR:-profile_out}
mkdir -p "$out"
timeout 900 rocprofv3 --kernel-trace --stats -d $out/prof_bench -o bench -- python bench.py --full > $out/${tag}_bench_rocprofv3.log 2>&1
grep -E '^\{"metric"' $out/${tag}_bench_rocprofv3.log > $out/${tag}_bench.json
python tools/rocpd_stats.py $out/prof_bench/bench_results.db --top 60 --split-grid msda_fwd_q64:1000 --csv $out/${tag}_bench_kernel_stats.csv > $out/${tag}_bench_kernel_stats.txt 2>&1
rm -rf $out/prof_bench
# one graph-replayed forward split into stages (no CPU baseline / parity pass in the trace)
timeout 600 rocprofv3 --kernel-trace -d $out/prof_fb -o fb -- python bench.py --no-cpu-baseline --extras 0 --steps 20 > /dev/null 2>&1
python tools/forward_breakdown.py $out/prof_fb/fb_results.db 14 > $out/${tag}_forward_breakdown.txt 2>&1
rm -rf $out/prof_fb
timeout 900 rocprofv3 --kernel-trace -d $out/prof_train -o train -- python bench.py --mode train --steps 8 --warmup 6 --no-cpu-baseline --no-kernel-probes > $out/${tag}_train_rocprofv3.log 2>&1
python tools/rocpd_stats.py $out/prof_train/train_results.db --last-ms 300 --top 60 > $out/${tag}_train_steady_state_kernel_stats.txt 2>&1
rm -rf $out/prof_train
tail -c 400 $out/${tag}_bench_rocprofv3.log | head -c 0
cat $out/${tag}_bench.json | cut -c1-900
grep -E '^\{"metric"' $out/${tag}_train_rocprofv3.log | cut -c1-330
head -4 $out/${tag}_train_steady_state_kernel_stats.txt | cut -c1-160
