"""B-multiply launches of a rocprofv3 --kernel-trace csv, per kernel instantiation and launch kind: single-slice launches (the
wraps) and the ten-slice chains of the stabilisation steps are told apart by duration (a chain takes > 3x the shortest launch of
its instantiation, or > SPLIT_US when given).
    python scripts/bmult_trace_split.py kernel_trace.csv [SPLIT_US]"""
import csv
import re
import sys

rows = {}
for r in csv.DictReader(open(sys.argv[1])):
    name = r.get("Kernel_Name") or r.get("Name") or ""
    m = re.search(r"k_bmult_(chain|direct)<([^>]*)>", name)
    if not m:
        continue
    dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    rows.setdefault(f"k_bmult_{m.group(1)}<{m.group(2)}>", []).append(dur)
for name in sorted(rows):
    d = sorted(rows[name])
    split = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0 * d[0]
    for kind, v in (("single", [x for x in d if x <= split]), ("chain", [x for x in d if x > split])):
        if v:
            print("%-46s %-6s calls %5d  mean %8.1f us  median %8.1f  min %8.1f  max %8.1f  total %8.1f ms" % (
                name, kind, len(v), sum(v) / len(v), v[len(v) // 2], v[0], v[-1], sum(v) / 1e3))
