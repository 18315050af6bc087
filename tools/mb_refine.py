"""The camera-and-points refinement launch (csrc/refine.hip: refine_kernel, then relative_pose_kernel) at the two shapes a
clip gives: T steps x 17 joints x 2 views refined per step (T groups of 17 points, one wave each) and as one clip (one
group of T x 17 points on one 512-thread workgroup), at lambda_x = 0, 1 and 100, linear and soft_l1.

Inputs: the rig of tests/refine_cases.py (1 px keypoint noise, joints 5 cm off), cameras started near the truth.

    python tools/mb_refine.py [--reps 10] [--steps 243] [--out result.json]

HIP events around each public call with a given start (output and workspace allocation + two launches + kernels), the
variants of one T interleaved (profiles/refine_points.md records a run).
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, nargs="+", default=[243])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import refine_cases as fc
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
        c = fc.rig(T=T, V=2, seed=100 + T)
        X, x2d, _ = fc.flat(c)
        Xd, xd, Kd = dev(X), dev(x2d), dev(c["K"])
        variants = {}
        for shape, per_step in (("per_step", True), ("clip", False)):
            R0, t0 = fc.start(c, per_step)
            for lambda_x, loss in ((0.0, "linear"), (1.0, "linear"), (100.0, "linear"), (100.0, "soft_l1")):
                kw = dict(K=Kd, R0=dev(R0), t0=dev(t0), group_size=fc.J if per_step else None, lambda_x=lambda_x, loss=loss,
                          f_scale=fc.F_SCALE)
                variants[f"{shape}_lx{lambda_x:g}_{loss}"] = lambda kw=kw: geometry.refine_cameras_points(Xd, xd, **kw)
        for fn in variants.values():         # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.reps):           # interleaved
            for k, fn in variants.items():
                ms[k].append(event_ms(fn))
        for k, fn in variants.items():
            r = fn()
            ne = r.n_evals.cpu().numpy()
            row = {"T": T, "variant": k, "groups": int(ne.size), "points_per_group": int(r.n_points.max()),
                   "call_ms_median": float(np.median(ms[k])), "call_ms_min": float(min(ms[k])), "call_ms_max": float(max(ms[k])),
                   "n_evals_median": float(np.median(ne)), "n_evals_max": int(ne.max()), "success": int(r.success.sum()),
                   "mean_err_px_median": float(np.median(r.mean_err.cpu().numpy())), "moved_median": float(np.median(r.moved.cpu().numpy()))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
           "note": "call = HIP events around geometry.refine_cameras_points with R0, t0 given (output + workspace allocation, "
                   "refine_kernel, relative_pose_kernel)"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
