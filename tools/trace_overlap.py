#!/usr/bin/env python3
"""Did two kernels of a rocprofv3 --kernel-trace CSV run at the same time?  For every dispatch of kernel A (a substring of its name) one line:
its duration, and how many microseconds of it lie inside the interval of the dispatch of another kernel that it shares the most time with
(its name, grid and duration).  usage: trace_overlap.py <kernel_trace.csv> <substring of A> [last N dispatches]
e.g. the averages beside the restricting relaxation launch: trace_overlap.py bench_kernel_trace.csv k_average_faces_all 20"""
import csv, sys
rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0],
         int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r.get("Grid_Size_Z", 1) or 1)) for r in csv.DictReader(open(sys.argv[1]))]
rows.sort()
mine = [r for r in rows if sys.argv[2] in r[2]]
if len(sys.argv) > 3: mine = mine[-int(sys.argv[3]):]
print("# dispatch of %s | its us | us of it inside another kernel's interval | that kernel | grid (work-items) | its us" % sys.argv[2])
tot = 0.0
for n, (a0, a1, name, grid) in enumerate(mine):
    best = (0, None)
    for b0, b1, other, g in rows:
        if b0 >= a1: break
        if b1 <= a0 or (b0, b1, other, g) == (a0, a1, name, grid): continue
        ov = min(a1, b1) - max(a0, b0)
        if ov > best[0]: best = (ov, (other, g, b1 - b0))
    tot += best[0] / 1e3
    if best[1]: print("%4d %8.1f %8.1f  %-48s %9d %8.1f" % (n, (a1 - a0) / 1e3, best[0] / 1e3, best[1][0][:48], best[1][1], best[1][2] / 1e3))
    else: print("%4d %8.1f %8.1f  (alone)" % (n, (a1 - a0) / 1e3, 0.0))
print("# mean overlap: %.1f us over %d dispatches" % (tot / max(len(mine), 1), len(mine)))
