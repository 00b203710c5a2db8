#!/usr/bin/env python3
"""The launches of a rocprofv3 --kernel-trace --output-format csv run in the order they were dispatched, one line each:
kernel name, grid (workgroups), workgroup size, LDS bytes.
usage: order_launch_list.py <dir with *kernel_trace.csv> > list.txt        (scripts/order_launch_sequence.py says what for)"""
import csv
import glob
import os
import sys

rows = []
for f in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(f) as fh:
        for r in csv.DictReader(fh):
            wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
            grid = [int(r["Grid_Size_" + a]) // max(w, 1) for a, w in zip("XYZ", wg)]  # the trace counts work-items
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
            rows.append((int(r["Dispatch_Id"]), f'{name}\tgrid {"x".join(map(str, grid))}\tworkgroup {"x".join(map(str, wg))}\tlds {r["LDS_Block_Size"]}'))
rows.sort()
for _, line in rows:
    print(line)
