"""The robust triangulation launch (csrc/geometry.hip: triangulate_robust_kernel) next to the plain DLT and the triage
launch at the same shapes, and the recovery table of its rules on the kernel's own outputs.

Shapes (T, V, J): (4, 2, 17), (4, 8, 17), (32, 8, 17), (4096, 8, 17); inputs: the arc rig of tests/robust_cases.py with
gross outliers (0 .. min(2, V - 3) views per joint moved by 25 .. 60 px), inlier_px = 3, five Gauss-Newton steps.

    python tools/mb_robust.py [--reps 20] [--out result.json]     HIP events around each call, the three interleaved
    rocprofv3 --kernel-trace --stats -d DIR -o robust --output-format csv -- python tools/mb_robust.py --kernel-only
    python tools/mb_robust.py --from-trace DIR/.../robust_kernel_trace.csv       kernel times per shape

--kernel-only launches, per shape, one warm-up and then --reps rounds of (robust, triage, plain) in that order, so the
trace's dispatches can be grouped by position.  profiles/robust_triangulation.md records a run.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

SHAPES = [(4, 2, 17), (4, 8, 17), (32, 8, 17), (4096, 8, 17)]
KERNELS = ("triangulate_robust_kernel", "triangulate_triage_kernel", "triangulate_dlt_kernel")
INLIER_PX = 3.0


def from_trace(path, reps):
    every = list(csv.DictReader(open(path)))
    out = []
    for name in KERNELS:
        rows = sorted((r for r in every if name in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
        per = reps + 1
        assert len(rows) == per * len(SHAPES), (name, len(rows), per)
        for k, (T, V, J) in enumerate(SHAPES):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[k * per + 1:(k + 1) * per]]
            out.append({"kernel": name, "T": T, "V": V, "J": J, "kernel_us_median": float(np.median(us)), "kernel_us_min": min(us),
                        "kernel_us_max": max(us)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--from-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.from_trace:
        res = {"source": "rocprofv3 --kernel-trace", "rows": from_trace(args.from_trace, args.reps)}
        print(json.dumps(res))
        if args.out:
            Path(args.out).write_text(json.dumps(res, indent=1))
        return
    import torch

    import robust_cases as rc
    from skiing_analysis_pytorch_amd import geometry

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    rows = []
    for T, V, J in SHAPES:
        c = rc.outlier_rig(V, J, 1000 * V + J, T=T)
        K, R, t, kp, conf = (dev(c[k]) for k in ("K", "R", "t", "kp", "conf"))
        calls = (lambda: geometry.triangulate_robust(K, R, t, kp, conf, inlier_px=INLIER_PX),
                 lambda: geometry.triangulate_triage(K, R, t, kp, conf),
                 lambda: geometry.triangulate_joints(K, R, t, kp))
        for fn in calls:      # warm-up
            fn()
        torch.cuda.synchronize()
        if args.kernel_only:
            for _ in range(args.reps):
                for fn in calls:
                    fn()
            torch.cuda.synchronize()
            continue
        ms = [[], [], []]
        for _ in range(args.reps):      # interleaved
            for k, fn in enumerate(calls):
                ms[k].append(event_ms(fn))
        row = {"T": T, "V": V, "J": J}
        for name, m in zip(("robust", "triage", "plain_dlt"), ms):
            row[f"{name}_call_ms_median"], row[f"{name}_call_ms_min"] = float(np.median(m)), float(min(m))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.kernel_only:
        return
    # the recovery table on the kernel's outputs: joint error against the true points, V = 8, J = 17, 64 steps
    c = rc.outlier_rig(8, 17, 817, T=64)
    K, R, t = (dev(c[k]) for k in ("K", "R", "t"))
    moved = c["moved"].any(axis=1)

    def err_mm(X):
        return np.linalg.norm(X.cpu().numpy().astype(np.float64) - c["X_true"], axis=-1) * 1e3

    table = {"plain_dlt": err_mm(geometry.triangulate_joints(K, R, t, dev(c["kp"]))),
             "robust_unrefined": err_mm(geometry.triangulate_robust(K, R, t, dev(c["kp"]), inlier_px=INLIER_PX, refine_iters=0).joints3d),
             "robust_refined": err_mm(geometry.triangulate_robust(K, R, t, dev(c["kp"]), inlier_px=INLIER_PX, refine_iters=5).joints3d),
             "unmoved_keypoints": err_mm(geometry.triangulate_robust(K, R, t, dev(c["clean"]), inlier_px=INLIER_PX, refine_iters=5).joints3d)}
    r = geometry.triangulate_robust(K, R, t, dev(c["kp"]), inlier_px=INLIER_PX)
    want = np.zeros(moved.shape, np.int64)
    for v in range(8):
        want |= (~c["moved"][:, v]).astype(np.int64) << v
    recovery = {"joints": int(moved.size), "joints_with_a_moved_view": int(moved.sum()),
                "inlier_set_is_exactly_the_unmoved_views": int((r.inlier_views.cpu().numpy() == want).sum()),
                "error_mm": {k: {"median": float(np.median(v)), "worst": float(v.max()), "median_moved": float(np.median(v[moved])),
                                 "worst_moved": float(v[moved].max())} for k, v in table.items()}}
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "inlier_px": INLIER_PX, "rows": rows, "recovery": recovery,
           "note": "call = HIP events around the public function (output allocation + launch + kernel), interleaved"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
