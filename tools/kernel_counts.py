#!/usr/bin/env python3
"""Summarise a `rocprofv3 --kernel-trace --stats` directory: total kernel launches and device time, then the top kernels.
usage: kernel_counts.py <prof dir> [rows]"""
import csv
import glob
import sys

f = glob.glob(sys.argv[1] + "/**/*kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(f[0])))
top = int(sys.argv[2]) if len(sys.argv) > 2 else 12
dur = lambda r: float(r["TotalDurationNs"]) if "TotalDurationNs" in r else int(r["Calls"]) * float(r["AverageNs"])
calls, total = sum(int(r["Calls"]) for r in rows), sum(dur(r) for r in rows)
print("kernels launched %d, distinct %d, device time %.3f ms" % (calls, len(rows), total / 1e6))
for r in rows[:top]:
    print("%-110s calls %6s avg_ns %12s pct %6s" % (r["Name"][:110], r["Calls"], r["AverageNs"], r["Percentage"]))
ot = [r for r in rows if "::ot_" in r["Name"]]
for r in ot:
    print("ncahip OT kernel: %-90s calls %6s avg_ns %12s total_ms %.3f" % (r["Name"][:90], r["Calls"], r["AverageNs"], dur(r) / 1e6))
