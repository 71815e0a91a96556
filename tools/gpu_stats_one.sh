#!/bin/bash
# rocprofv3 --kernel-trace of ONE bench --full configuration -> $BENCH_OUT/TAG_kernel_stats.txt, default out/
#   (bash tools/gpu_stats_one.sh TAG [bench args ...])
set -u; R=$PWD; TAG=$1; shift; mkdir -p "${BENCH_OUT:-out}"; OUT=$(cd "${BENCH_OUT:-out}" && pwd)
cd /tmp; export TMPDIR=/tmp PYTHONUNBUFFERED=1
timeout 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o bench -- python $R/bench.py --full --no-cpu-baseline --no-alt-precision --no-teacher-forced --no-other-configs "$@" > $OUT/${TAG}_rocprof_bench.json 2> $OUT/${TAG}_rocprof.err
python $R/tools/rocprof_summary.py $OUT/prof_$TAG/bench_results.db $OUT/${TAG}_kernel_stats.txt > /dev/null
rm -rf $OUT/prof_$TAG; head -n 30 $OUT/${TAG}_kernel_stats.txt | cut -c1-220
