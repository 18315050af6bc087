"""The camera resection launch (csrc/resect.hip: resect_kernel + relative_pose_kernel) at the two shapes a clip gives:
T steps x 17 joints x 2 views solved per step (T x 2 problems of 17 points, one wave each) and as one clip (2 problems
of T x 17 points, one 1024-thread workgroup each), linear and soft_l1.

Inputs: the rig of tests/resect_cases.py, 1 px noise; the soft_l1 rows add 5 % keypoints moved by sigma = 80 px.

    python tools/mb_resect.py [--reps 20] [--steps 4096 64] [--out result.json]

HIP events around each public call (output allocation + two launches + kernels), the variants of one T interleaved
(profiles/resection.md records a run and sets the times beside the VGGT step they would replace).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, nargs="+", default=[4096, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import resect_cases as rc
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
    for T in args.steps:
        variants = {}
        for loss, outliers in (("linear", 0.0), ("soft_l1", 0.05)):
            c = rc.rig(T=T, V=2, seed=100 + T, noise=1.0, outliers=outliers)
            X, x2d, _ = rc.flat(c)
            Xd, xd, Kd = dev(X), dev(x2d), dev(c["K"])
            for shape, gs in (("per_step", rc.J), ("clip", None)):
                kw = dict(K=Kd, group_size=gs, loss=loss, f_scale=rc.F_SCALE)
                variants[f"{shape}_{loss}"] = (c, lambda Xd=Xd, xd=xd, kw=kw: geometry.resect_cameras(Xd, xd, **kw))
        for _, fn in variants.values():      # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.reps):           # interleaved
            for k, (_, fn) in variants.items():
                ms[k].append(event_ms(fn))
        for k, (c, fn) in variants.items():
            r = fn()
            ne = r.n_evals.cpu().numpy()
            d = rc.pose_distance(r.R.cpu().numpy(), r.t.cpu().numpy(), c["R"], c["t"])
            row = {"T": T, "variant": k, "problems": int(ne.size), "points_per_problem": int(r.n_points.max()),
                   "call_ms_median": float(np.median(ms[k])), "call_ms_min": float(min(ms[k])), "call_ms_max": float(max(ms[k])),
                   "n_evals_median": float(np.median(ne)), "n_evals_max": int(ne.max()), "success": int(r.success.sum()),
                   "pose_distance_median": float(np.median(d)), "mean_err_px_median": float(np.median(r.mean_err.cpu().numpy()))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
           "note": "call = HIP events around geometry.resect_cameras (output allocation + resect_kernel + relative_pose_kernel)"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
