#!/usr/bin/env python3
"""Are two runs' kernel dispatches the same?  Compares the rocprofv3 kernel traces of two runs of one command, e.g. the
rollout-facing GPU tests on two builds of libses_hip.so (SES_LIB_PATH): every host-side path computes the same bits by design,
so only the trace shows whether the host still SELECTS the same kernels.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_A -- python -m pytest ...      (and the same into DIR_B)
    python tools/dispatch_trace_compare.py DIR_A DIR_B > profiles/dispatch_trace_equal.txt

Per kernel name: the dispatch counts of both runs; then whether the sets of distinct (kernel, grid, workgroup, LDS bytes)
tuples are equal.  Exit status 1 when anything differs.
"""
import collections
import csv
import glob
import os
import sys


def load(d):
    counts, shapes = collections.Counter(), set()
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                counts[name] += 1
                shapes.add((name, tuple(int(row[f"Grid_Size_{a}"]) for a in "XYZ"),
                            tuple(int(row[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(row["LDS_Block_Size"])))
    return counts, shapes


def main(a, b):
    (ca, sa), (cb, sb) = load(a), load(b)
    bad = 0
    print(f"# kernel dispatches, A = {a}, B = {b}: count A, count B, equal?, kernel")
    for name in sorted(set(ca) | set(cb)):
        same = ca[name] == cb[name]
        bad += not same
        print(f"{ca[name]:8d} {cb[name]:8d} {'equal' if same else 'NOT EQUAL'}  {name[:150]}")
    print(f"# {len(set(ca) | set(cb))} kernel names, {sum(ca.values())} / {sum(cb.values())} dispatches, {bad} names with different counts")
    print(f"# distinct (kernel, grid, workgroup, LDS bytes) tuples: {len(sa)} / {len(sb)}, sets {'equal' if sa == sb else 'NOT EQUAL'}")
    for t in sorted(sa ^ sb):
        print(f"#   only in {'A' if t in sa else 'B'}: {t}")
    return 1 if bad or sa != sb else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
