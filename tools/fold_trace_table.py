"""Where the DPT heads' levels 0 / 1 go in a bench-step kernel trace, SKIMI_DPT_FOLD=0 against =1.
usage: fold_trace_table.py <kernel_trace.csv of =0> <kernel_trace.csv of =1>

Groups (summed kernel time of the whole trace, ms):
  levels 0 / 1 : =0: the ConvTranspose pixel-shuffle GEMMs (gemm_x3w4_kernel<0> launches of 16 or 8 column tiles per row tile,
                 found by their grid) with the split passes and the layer_rn 3x3 conv that follow each on its queue, and the
                 add_uv_pos passes of those two levels; =1: gemm_x3w4_kernel<3> and add_uv_pos_records_kernel
  x3 head      : every gemm_x3w4 / gemm_x3w4n / conv_direct_n32 kernel, split_records and add_uv_pos* (levels 0 / 1 included)
  other        : everything else"""
import collections
import csv
import sys


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"].replace("void ", "").replace("skimi::", "").split("(")[0]
        rows.append(dict(name=n, q=r.get("Queue_Id", "0"), t0=int(r["Start_Timestamp"]), d=int(r["End_Timestamp"]) - int(r["Start_Timestamp"]),
                         wgs=int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))))
    rows.sort(key=lambda r: r["t0"])
    return rows


def is_head(n):
    return n.startswith(("gemm_x3w4", "conv_direct_n32", "split_records", "add_uv_pos"))


def groups(rows):
    lvl = collections.Counter()
    byq = collections.defaultdict(list)
    for r in rows:
        byq[r["q"]].append(r)
    # row tiles of the coarse map = the grid of the narrowest projection (256 columns = one column tile)
    ntm = min((r["wgs"] for r in rows if r["name"].startswith("gemm_x3w4_kernel<0")), default=0)
    for q in byq.values():
        for i, r in enumerate(q):
            if r["name"].startswith(("gemm_x3w4_kernel<3", "add_uv_pos_records")):
                lvl[r["name"]] += r["d"]
            elif r["name"].startswith("gemm_x3w4_kernel<0") and r["wgs"] in (16 * ntm, 8 * ntm):
                # on its queue: add_uv_pos, split_records, THIS ConvTranspose GEMM, split_records, layer_rn conv
                want = {i - 2: "add_uv_pos_kernel", i - 1: "split_records", i: "gemm_x3w4_kernel<0", i + 1: "split_records",
                        i + 2: "gemm_x3w4_kernel<2"}
                for j, pre in want.items():
                    if 0 <= j < len(q) and q[j]["name"].startswith(pre):
                        lvl[("convT " if j == i else "layer_rn " if j == i + 2 else "") + pre] += q[j]["d"]
                    else:
                        print(f"warning: expected {pre} next to a ConvTranspose launch, found {q[j]['name'] if 0 <= j < len(q) else None}")
    head = sum(r["d"] for r in rows if is_head(r["name"]))
    pack = sum(r["d"] for r in rows if r["name"].startswith("dpt_fold_"))   # weight folding, once when the model is created
    total = sum(r["d"] for r in rows) - pack
    return lvl, head, total, pack


res = [groups(load(p)) for p in sys.argv[1:3]]
for tag, (lvl, head, total, pack) in zip(("SKIMI_DPT_FOLD=0", "SKIMI_DPT_FOLD=1"), res):
    print(f"{tag}: levels 0 / 1 {sum(lvl.values()) / 1e6:8.2f} ms | x3 head kernels {head / 1e6:8.2f} ms | other {(total - head) / 1e6:8.2f} ms | "
          f"all {total / 1e6:8.2f} ms | (weight folding at create, not in the step: {pack / 1e6:.2f} ms)")
    for k, v in sorted(lvl.items()):
        print(f"    {k:40s} {v / 1e6:8.2f} ms")
