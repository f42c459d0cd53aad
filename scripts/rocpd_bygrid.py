#!/usr/bin/env python3
"""per-(kernel, grid) breakdown of a rocprofv3 rocpd database: ms per step.  short() / launch_key() / launches() are shared with
scripts/launch_coverage.py"""
import re
import sqlite3
import sys


def short(name):
    """kernel name without namespaces, return type and argument list (template arguments kept)"""
    s = name.replace("(anonymous namespace)::", "").replace("aclgan::", "").replace("void ", "")
    return re.sub(r"\(.*$", "", s)


def launch_key(name, gx, gy, gz, wx):
    """(kernel, workgroups along x, grid y, grid z) of one launch"""
    return (short(name), gx // wx, gy, gz)


def launches(path):
    """[(launch key, start, end)] of every kernel launch in the database"""
    cur = sqlite3.connect(path).cursor()
    return [(launch_key(name, gx, gy, gz, wx), s, e)
            for name, s, e, gx, gy, gz, wx in cur.execute("select name, start, end, grid_x, grid_y, grid_z, workgroup_x from kernels")]


def main():
    steps = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
    pat = sys.argv[3] if len(sys.argv) > 3 else "conv_"
    agg = {}
    for k, s, e in launches(sys.argv[1]):
        if pat not in k[0]:
            continue
        a = agg.setdefault(k, [0, 0]); a[0] += 1; a[1] += e - s
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1][1])[:int(sys.argv[4]) if len(sys.argv) > 4 else 40]:
        print("%-38s blocks=%6d y=%d z=%3d calls/step=%6.1f ms/step=%7.2f avg_us=%8.1f" % (k[0], k[1], k[2], k[3], a[0] / steps, a[1] / steps / 1e6, a[1] / a[0] / 1e3))


if __name__ == "__main__":
    main()
