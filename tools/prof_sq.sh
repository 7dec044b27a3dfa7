#!/bin/bash
# SQ counters of the fused rollout kernel (two passes of <= 8 SQ counters), kernel-trace only.
# SQ_BENCH_LEGS="" profiles the lean headline run only: then the one rollout kernel in the passes is the headline's, which is
# the one tools/collect_sq.py must put at the top level of profiles/rNN_sq_rollout.json (bench.py reads it from there).
cd /tmp && export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=${PROF_OUT:-$R/prof_out}      # raw rocprofv3 output (git-ignored)
mkdir -p $OUT
i=0
for set in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" \
           "SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_SALU SQ_THREAD_CYCLES_VALU"; do
  i=$((i+1))
  rm -rf $OUT/sq_$i
  rocprofv3 --pmc $set --kernel-trace --output-format csv -d $OUT/sq_$i -- python3 $R/bench.py ${SQ_BENCH_LEGS---full --no-cpu-baseline --no-roofline} --steps 3 --warmup 1 "$@" > $OUT/sq_$i.log 2>&1
  f=$(find $OUT/sq_$i -name "*counter_collection.csv" | head -1)
  python3 - "$f" <<'PY'
import csv, sys, collections
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(sys.argv[1])):
    k = r["Kernel_Name"].split("(")[0]
    if "rollout" in k:
        agg[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
for k, d in agg.items():
    print(k)
    for c, v in sorted(d.items()):
        print(f"   {c:26s} avg per dispatch = {sum(v)/len(v):16.1f}  (n={len(v)})")
PY
done
