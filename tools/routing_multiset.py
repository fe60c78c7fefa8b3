#!/usr/bin/env python3
"""(kernel with template arguments, workgroups x threads, LDS bytes) -> launches of a rocprofv3 --kernel-trace --output-format csv run,
one sorted line each: two commits route alike when `diff` of their outputs is empty (profiles/r08_routing_diff.txt).
usage: routing_multiset.py <dir with *_kernel_trace.csv>"""
import collections
import csv
import glob
import sys


def main():
    g = collections.Counter()
    for f in glob.glob(sys.argv[1] + "/**/*_kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            wg = max(int(r["Workgroup_Size_X"]), 1)
            g[(r["Kernel_Name"][:112], int(r["Grid_Size_X"]) // wg, wg, int(r["LDS_Block_Size"]))] += 1
    for (name, wgs, wg, lds), n in sorted(g.items()):
        print("%-112s wgs %6d x %4d  lds %6d  launches %5d" % (name, wgs, wg, lds, n))


if __name__ == "__main__":
    main()
