"""Where output_conv1 of the DPT heads goes in a bench-step kernel trace, SKIMI_DPT_OC1_COARSE=0 against =1.
usage: oc1_trace_table.py <kernel_trace.csv of =0> <kernel_trace.csv of =1>

Groups (summed kernel time of the whole trace, ms), found by the launches' order on their queue:
  output_conv1 : =0: every bilinear_ac_planes_kernel launch (the x2 upsample into records), the gemm_x3w4_kernel<0> in front of
                 it (refinenet1's out_conv, fp32 rows out) and the gemm_x3w4n_kernel<2> behind it (the 3x3 conv on the fine map);
                 =1: every dpt_tap_sum_kernel launch and the two gemm_x3w4_kernel<0> in front of it (out_conv, records out, and
                 the nine taps' contraction)
  x3 head      : every gemm_x3w4 / gemm_x3w4n / conv_direct_n32 kernel, split_records, add_uv_pos*, bilinear_ac_planes and
                 dpt_tap_sum (output_conv1 included)
  other        : everything else"""
import collections
import csv
import sys


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"].replace("void ", "").replace("skimi::", "").split("(")[0]
        rows.append(dict(name=n, q=r.get("Queue_Id", "0"), t0=int(r["Start_Timestamp"]), d=int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort(key=lambda r: r["t0"])
    return rows


def is_head(n):
    return n.startswith(("gemm_x3w4", "conv_direct_n32", "split_records", "add_uv_pos", "bilinear_ac_planes", "dpt_tap_sum"))


def groups(rows):
    oc1, count = collections.Counter(), collections.Counter()
    byq = collections.defaultdict(list)
    for r in rows:
        byq[r["q"]].append(r)
    for q in byq.values():
        for i, r in enumerate(q):
            if r["name"].startswith("bilinear_ac_planes_kernel"):
                want = {i - 1: ("out_conv ", "gemm_x3w4_kernel<0"), i: ("", "bilinear_ac_planes_kernel"), i + 1: ("3x3 conv ", "gemm_x3w4n_kernel<2")}
            elif r["name"].startswith("dpt_tap_sum_kernel"):
                want = {i - 2: ("out_conv ", "gemm_x3w4_kernel<0"), i - 1: ("taps ", "gemm_x3w4_kernel<0"), i: ("", "dpt_tap_sum_kernel")}
            else:
                continue
            for j, (tag, pre) in want.items():
                if 0 <= j < len(q) and q[j]["name"].startswith(pre):
                    oc1[tag + pre] += q[j]["d"]
                    count[tag + pre] += 1
                else:
                    print(f"warning: expected {pre} at {j - i:+d} of {r['name']}, found {q[j]['name'] if 0 <= j < len(q) else None}")
    head = sum(r["d"] for r in rows if is_head(r["name"]))
    total = sum(r["d"] for r in rows)
    return oc1, count, head, total


res = [groups(load(p)) for p in sys.argv[1:3]]
for tag, (oc1, count, head, total) in zip(("SKIMI_DPT_OC1_COARSE=0", "SKIMI_DPT_OC1_COARSE=1"), res):
    print(f"{tag}: output_conv1 {sum(oc1.values()) / 1e6:8.2f} ms | x3 head kernels {head / 1e6:8.2f} ms | other {(total - head) / 1e6:8.2f} ms | "
          f"all {total / 1e6:8.2f} ms")
    for k, v in sorted(oc1.items()):
        print(f"    {k:40s} {v / 1e6:8.2f} ms in {count[k]} launches")
