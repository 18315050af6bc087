"""The camera calibration call (csrc/calibrate.hip: the object-point copy, bev.hip's homography fit, calibrate_kernel) at
three shapes: one calibration of V = 24 views, one of V = 181 views (the size of the calibration the reference ships), and
G = 64 view subsets of the V = 24 problem (a bootstrap: every group drops a random sixth of the views), rational model,
9 x 6 board, 0.1 px corner noise.  Beside each, scipy's least_squares(method="lm") on the same residual from the same start
on the host (one problem; for G = 64 the time of one subset times 64): scipy, not cv2, which is not installed.

Inputs: the fixture of tests/calibrate_cases.py; the 181 poses are its 24 poses perturbed (seeded).

    python tools/mb_calibrate.py [--reps 10] [--out result.json] [--no-scipy]

HIP events around each public call (output and workspace allocation + three launches), the variants interleaved, the
median of `reps` after a warm-up (profiles/calibrate.md records a run).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import torch

    import calibrate_cases as cc
    import calibrate_restated as cr
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

    f = cc.fixture()
    obj = cc.prepare_object_points((9, 6), float(f["square"]))
    p = cc.true_params()
    rng = np.random.default_rng(7)

    def corners(rvecs, tvecs):
        img = np.stack([cr.project(p, cc.rodrigues(r), t, obj) for r, t in zip(rvecs, tvecs)])
        return img + 0.1 * rng.normal(0, 1, img.shape)

    pick = rng.integers(0, 24, 181)
    img24 = corners(f["rvecs"], f["tvecs"])
    img181 = corners(f["rvecs"][pick] + 0.05 * rng.normal(0, 1, (181, 3)), f["tvecs"][pick] * (1 + 0.05 * rng.normal(0, 1, (181, 3))))
    use64 = (rng.uniform(0, 1, (64, 24)) > 1 / 6).astype(np.uint8)
    objd, d24, d181, u64 = dev(obj), dev(img24), dev(img181), dev(use64)
    variants = {"V24_G1": lambda: geometry.calibrate_camera(objd, d24, cc.SIZE),
                "V181_G1": lambda: geometry.calibrate_camera(objd, d181, cc.SIZE),
                "V24_G64": lambda: geometry.calibrate_camera(objd, d24, cc.SIZE, use=u64)}
    for fn in variants.values():         # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.reps):           # interleaved
        for k, fn in variants.items():
            ms[k].append(event_ms(fn))

    def scipy_ms(img, use):
        from test_calibrate_cpu import scipy_solve
        mask = cr.free_mask()
        views = [v for v in range(img.shape[0]) if use is None or use[v]]
        Hn, _ = cr.homographies(obj, img)
        p0 = np.zeros(12)
        p0[:4] = cr.start_intrinsics(Hn, views, *cc.SIZE)
        poses = {v: cr.start_pose(p0, Hn[v]) for v in views}
        t0 = time.perf_counter()
        _, _, cost = scipy_solve(dict(obj=obj, img=img), mask, p0, poses, np.isfinite(img).all(-1))
        return (time.perf_counter() - t0) * 1e3, cost

    rows = []
    for k, fn in variants.items():
        r = fn()
        ne = r.n_evals.cpu().numpy()
        row = {"variant": k, "groups": int(ne.size), "views": int(r.n_views.max()), "call_ms_median": float(np.median(ms[k])),
               "call_ms_min": float(min(ms[k])), "call_ms_max": float(max(ms[k])), "n_evals_median": float(np.median(ne)),
               "n_evals_max": int(ne.max()), "success": int(r.success.sum()), "rms_median": float(np.median(r.rms.cpu().numpy()))}
        if not args.no_scipy:
            img, use = (img181, None) if k == "V181_G1" else (img24, use64[0] if k == "V24_G64" else None)
            t, cost = scipy_ms(img, use)
            row["scipy_lm_host_ms"] = t * (64 if k == "V24_G64" else 1)
            row["scipy_lm_note"] = "one subset x 64" if k == "V24_G64" else "one problem"
            row["scipy_cost_minus_kernel_cost"] = float(cost - r.cost.cpu().numpy()[0])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
           "note": "call = HIP events around geometry.calibrate_camera (output + workspace allocation, the object-point copy, "
                   "homography_fit_kernel, calibrate_kernel); scipy = least_squares(method='lm') on the host, not cv2"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
