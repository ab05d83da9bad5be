# the main stream's kernel sequence per batch in a kernel trace: the queue that runs the aggregation, its most common cycle of
# kernel names, each kernel's average over the last 200 such cycles and the gaps between its kernels (profiles/r15/*_summary.txt)
#   python3 tools/exp/main_sequence.py kt_kernel_trace.csv
import csv, sys
from collections import Counter
import numpy as np
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
short = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
q = Counter(r["Queue_Id"] for r in rows if "k_fc1_agg_reg" in r["Kernel_Name"]).most_common(1)[0][0]
main = [r for r in rows if r["Queue_Id"] == q]
names = [short(r) for r in main]
idx = [i for i, n in enumerate(names) if n.startswith("k_fc1_agg_reg")]
cyc = Counter(tuple(names[a:b]) for a, b in zip(idx[:-1], idx[1:]))
print("main stream (queue %s): %d kernels; cycles between aggregations:" % (q, len(main)))
for c, n in cyc.most_common(4):
    print("  %5d x  %s" % (n, " -> ".join(c)))
best = cyc.most_common(1)[0][0]
segs = [(a, b) for a, b in zip(idx[:-1], idx[1:]) if tuple(names[a:b]) == best][-200:]
st = lambda r: int(r["Start_Timestamp"]) / 1e3
en = lambda r: int(r["End_Timestamp"]) / 1e3
for j, n in enumerate(best):
    print("  %-28s %7.1f us avg (last %d cycles)" % (n, np.mean([en(main[a + j]) - st(main[a + j]) for a, b in segs]), len(segs)))
for j in range(len(best) - 1):
    print("  gap %d -> %d %7.1f us median" % (j, j + 1, np.median([st(main[a + j + 1]) - en(main[a + j]) for a, b in segs])))
print("  aggregation start -> next aggregation start %7.1f us median" % np.median([st(main[b]) - st(main[a]) for a, b in segs]))
print("  aggregation start -> end of the cycle's last kernel %7.1f us median" % np.median([en(main[b - 1]) - st(main[a]) for a, b in segs]))
