"""Where the DPT heads' tail goes in a bench-step kernel trace (rocprofv3 --kernel-trace --stats --output-format csv of
`bench.py --steps 2 --warmup 1`), one line per trace.  usage: tail_trace_table.py <kernel_trace.csv> [<kernel_trace.csv> ...]

  tail  : conv_direct_n32* + bilinear_ac_planes_kernel launches at the full-size map (the tail's upsample writes [hi C | lo C]
          pixel records; the heads' other bilinear_ac_planes launch, into slice records at the half-size map, is told apart by
          its smaller grid and counted with the rest: give the trace of the two-launch tail along with the fused one)
  other : every other kernel of the trace"""
import collections
import csv
import sys


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"].replace("void ", "").replace("skimi::", "").split("(")[0]
        rows.append((n, int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r["Grid_Size_Y"])))
    return rows


traces = {path: load(path) for path in sys.argv[1:]}
# the tallest bilinear_ac_planes grid of all the traces given: a trace of the fused tail has none of that height
ymax = max((y for rows in traces.values() for n, _, y in rows if n.startswith("bilinear_ac_planes")), default=0)
for path, rows in traces.items():
    per = collections.defaultdict(lambda: [0, 0])
    other = 0
    for n, d, y in rows:
        if n.startswith("conv_direct_n32") or (n.startswith("bilinear_ac_planes") and y == ymax):
            per[n][0] += d
            per[n][1] += 1
        else:
            other += d
    tail = sum(v[0] for v in per.values())
    print(f"{path}: tail {tail / 1e6:8.2f} ms | other {other / 1e6:8.2f} ms | all {(tail + other) / 1e6:8.2f} ms")
    for n, (d, k) in sorted(per.items()):
        print(f"    {n:45s} {d / 1e6:8.2f} ms in {k:3d} launches = {d / k / 1e3:8.1f} us each")
