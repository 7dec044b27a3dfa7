#!/bin/bash
# rocprofv3 kernel trace of the default bench command; summaries land in $PROF_OUT (default prof_out/)
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${PROF_OUT:-$R/prof_out}      # raw rocprofv3 output (git-ignored)
mkdir -p $OUT
rm -rf $OUT/prof_kt
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_kt -- python3 $R/bench.py --full --no-cpu-baseline "$@" > $OUT/prof_kt_bench.log 2>&1
grep "^{\"metric\"" $OUT/prof_kt_bench.log | tail -1 | cut -c1-300
find $OUT/prof_kt -name "*kernel_stats.csv" | head -1 | xargs -I{} sh -c 'cp {} '$OUT'/kernel_stats.csv; head -20 {}'
