"""The essential-matrix RANSAC call (csrc/essential.hip: prep, hypotheses, score and finish kernels) at the two shapes a
243-frame clip gives: the whole clip as one group (4131 correspondences) at 1024 hypotheses, and 243 per-frame groups of
17 at 256 hypotheses each.

Inputs: the rig of tests/resect_cases.py, 1 px noise, 10 % keypoints moved by sigma = 80 px.

    python tools/mb_essential.py [--reps 20] [--frames 243] [--out result.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mb_essential.py --reps 5

HIP events around each public call (output and workspace allocation + four launches), the two shapes interleaved; the
share of the scoring launch comes from the kernel trace of the second command (profiles/essential.md).
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
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import essential_cases as ec
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

    T = args.frames
    p = ec.pair(rc.rig(T=T, V=2, seed=100 + T, noise=1.0, outliers=0.10))
    x2d, K = dev(p["x2d"]), dev(p["K"])
    variants = {
        "clip_H1024": dict(group_size=None, hypotheses=1024, seed=1 << 20),
        "per_frame_H256": dict(group_size=rc.J, hypotheses=256, seed=1 << 20),
    }
    fns = {k: (lambda kw=kw: geometry.essential_ransac(x2d, K, **kw)) for k, kw in variants.items()}
    for fn in fns.values():      # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.reps):   # interleaved
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    rows = []
    for k, fn in fns.items():
        r = fn()
        ok = r.success.cpu().numpy()
        R, t = r.R.cpu().numpy()[ok], r.t.cpu().numpy()[ok]
        rot = [ec.rotation_angle_deg(Rg, p["R"]) for Rg in R]
        tdir = [ec.direction_angle_deg(tg, p["t"]) for tg in t]
        row = {"frames": T, "variant": k, "groups": int(ok.size), "points_per_group": int(r.n_used.max()),
               "hypotheses": variants[k]["hypotheses"], "solutions_per_group_median": float(np.median(r.n_solutions.cpu().numpy())),
               "sampson_errors_per_call": float((r.n_solutions.double() * r.n_used.double()).sum()),
               "call_ms_median": float(np.median(ms[k])), "call_ms_min": float(min(ms[k])), "call_ms_max": float(max(ms[k])),
               "success": int(ok.sum()), "inlier_ratio_median": float(np.median((r.n_inliers / r.n_used.clamp(min=1)).cpu().numpy())),
               "rotation_err_deg_median": float(np.median(rot)), "translation_dir_err_deg_median": float(np.median(tdir))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
           "note": "call = HIP events around geometry.essential_ransac (output + workspace allocation, prep, hypotheses, score, finish)"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
