#!/usr/bin/env python3
"""(kernel, blocks, y, z) launches of trace(s) A that trace(s) B never made -- e.g. A = the kernel traces of the bench step per workload
(scripts/trace_step.sh), B = a kernel trace of the operator tests.  The launch key is scripts/rocpd_bygrid.py's (imported from it).

usage: python scripts/launch_coverage.py A1.db[,A2.db ...] B1.db[,B2.db ...] [regex of kernel names]
       default regex: the convolution (fold gathers included), Winograd, normalisation and split-K / weight-gradient finish kernels, and the
       reductions whose plan depends on the deterministic mode: ordered column sums, ordered slice sums, the O-sliced linear input gradient"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rocpd_bygrid import launches  # noqa: E402

DEFAULT = r"conv_|wino_|norm_|fwd_split_finish|wgrad_.*finish|colsum|reduce_slices|linear_dx"


def counts(paths):
    """{launch key: calls} over every database in paths"""
    out = {}
    for p in paths:
        for k, _, _ in launches(p):
            out[k] = out.get(k, 0) + 1
    return out


def main():
    a, b = sys.argv[1].split(","), sys.argv[2].split(",")
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else DEFAULT)
    la, lb = counts(a), counts(b)
    sel = sorted(k for k in la if pat.search(k[0]))
    missing = [k for k in sel if k not in lb]
    print("# %d distinct (kernel, blocks, y, z) launches in A match /%s/; %d of them are not in B" % (len(sel), pat.pattern, len(missing)))
    for k in missing:
        print("%-60s blocks=%6d y=%4d z=%4d calls=%d" % (k[0][:60], k[1], k[2], k[3], la[k]))


if __name__ == "__main__":
    main()
