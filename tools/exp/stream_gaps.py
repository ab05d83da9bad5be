# k_stream's launches in a rocprofv3 kernel trace of a bench run (profiles/rN/*c5_stream_gaps.txt): the kernel's time over
# the last n launches (the timed region's four-batch launches), the distance from the end of one to the start of the next,
# and every kernel's average over its last 200 launches.
#   python3 tools/exp/stream_gaps.py kt_kernel_trace.csv [50]
import csv, sys
from collections import defaultdict
import numpy as np
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ks = np.array([(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if "k_stream" in r["Kernel_Name"]][-n:]) / 1e3
dur = ks[:, 1] - ks[:, 0]
gap = ks[1:, 0] - ks[:-1, 1]
s2s = np.diff(ks[:, 0])
print("k_stream, the last %d launches (the timed region's four-batch launches): kernel %.1f us median (%.1f mean); end of one -> start of "
      "the next %.1f us median (10 %% %.1f, 90 %% %.1f, mean %.1f); start to start %.1f us median = %.1f us per batch" % (
          n, np.median(dur), dur.mean(), np.median(gap), np.percentile(gap, 10), np.percentile(gap, 90), gap.mean(),
          np.median(s2s), np.median(s2s) / 4))
by = defaultdict(list)
for r in rows:
    by[r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
print("%-36s %5s %10s" % ("kernel (last 200 launches)", "calls", "avg us"))
for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1]))[:24]:
    print("%-36s %5d %10.1f" % (name[:34], len(v), np.mean(v[-200:]) / 1e3))
