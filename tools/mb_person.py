"""The person origin on the device (csrc/person.hip, geometry.person_origin) against the host stage it replaces
(`wp.cpu().numpy()` + multi_view_process.extract_person_points per map), and the triage launch.

Maps: M = 8 and 32 of 518 x 518 (person depth 5 +- 0.4, 30 % background at 20 +- 3, 1 % NaN, 0.5 % inf), boxes in a
1080 x 1920 source: "typical" (~ 200 x 400 source pixels at random positions) and the full frame.

    python tools/mb_person.py [--reps 5] [--out result.json]          HIP events around the call + the host path
    rocprofv3 --kernel-trace --stats -d DIR -o person --output-format csv -- python tools/mb_person.py --kernel-only
    python tools/mb_person.py --from-trace DIR/.../person_kernel_trace.csv      kernel times per configuration

--kernel-only launches every configuration --reps times in a fixed order after one warm-up launch each, so the trace's
person_origin_kernel dispatches can be grouped by position.  profiles/person_triage.md records a run.
"""
from __future__ import annotations

import argparse
import csv
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

SOURCE = (1080, 1920)
CONFIGS = [(8, "typical"), (8, "full"), (32, "typical"), (32, "full")]


def scene(M, kind, seed=0, H=518, W=518):
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, 1.0, (M, H, W, 3)).astype(np.float32)
    z = rng.normal(5.0, 0.4, (M, H, W))
    bg = rng.random((M, H, W)) < 0.30
    z[bg] = rng.normal(20.0, 3.0, int(bg.sum()))
    P[..., 2] = z.astype(np.float32)
    flat = P.reshape(-1)
    flat[rng.random(flat.size) < 0.01] = np.nan
    flat[rng.random(flat.size) < 0.005] = np.inf
    if kind == "full":
        boxes = np.tile(np.array([0, 0, SOURCE[1], SOURCE[0]], np.float32), (M, 1))
    else:
        x = rng.uniform(0, SOURCE[1] - 200, M)
        y = rng.uniform(0, SOURCE[0] - 400, M)
        boxes = np.stack([x, y, x + 200, y + 400], axis=1).astype(np.float32)
    return P, boxes


def from_trace(path, reps):
    every = list(csv.DictReader(open(path)))
    dur = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in every if name in r["Kernel_Name"]]   # noqa: E731
    small = {name: float(np.median(dur(name)[1:])) for name in ("triangulate_triage_kernel", "triangulate_dlt_kernel") if dur(name)}
    rows = [r for r in every if "person_origin_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = reps + 1
    assert len(rows) == per * len(CONFIGS), (len(rows), per, len(CONFIGS))
    out = []
    for k, (M, kind) in enumerate(CONFIGS):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[k * per + 1:(k + 1) * per]]
        out.append({"M": M, "boxes": kind, "kernel_us_median": float(np.median(us)), "kernel_us_min": min(us), "kernel_us_max": max(us)})
    return out + [{"kernel": k, "T": 4, "V": 2, "J": 17, "kernel_us_median": v} for k, v in small.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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

    from skiing_analysis_pytorch_amd import geometry
    from skiing_analysis_pytorch_amd import multi_view_process as mv

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    rows = []
    for M, kind in CONFIGS:
        P, boxes = scene(M, kind)
        Pd, bd = torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda()
        got = geometry.person_origin(Pd, bd, SOURCE)        # warm-up
        torch.cuda.synchronize()
        if args.kernel_only:
            for _ in range(args.reps):
                geometry.person_origin(Pd, bd, SOURCE)
            torch.cuda.synchronize()
            continue
        dev, host = [], []
        for _ in range(args.reps):      # interleaved
            dev.append(event_ms(lambda: geometry.person_origin(Pd, bd, SOURCE)))
            t0 = time.perf_counter()
            wp = Pd.cpu().numpy()
            t1 = time.perf_counter()
            pts = [mv.extract_person_points(wp[m], boxes[m], SOURCE) for m in range(M)]
            origins = [p.mean(axis=0) for p in pts]
            t2 = time.perf_counter()
            host.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
        kept = got.n_kept.cpu().numpy()
        assert [len(p) for p in pts] == kept.tolist(), "the device kept other points than the host path"
        diff = float(np.abs(np.stack(origins).astype(np.float64) - got.origin.cpu().numpy()).max())
        row = {"M": M, "boxes": kind, "points_in_box_mean": float(got.stats[:, 0].mean()),
               "device_call_ms_median": float(np.median(dev)), "host_copy_ms_median": float(np.median([h[0] for h in host])),
               "host_numpy_ms_median": float(np.median([h[1] for h in host])), "origin_max_abs_diff_vs_host_f32": diff}
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the triage launch at T J = 4 x 17, two views
    rng = np.random.default_rng(1)
    T, V, J = 4, 2, 17
    K = torch.tensor([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]]).repeat(T, V, 1, 1).cuda()
    R = torch.eye(3).repeat(T, V, 1, 1).cuda()
    t = torch.from_numpy(rng.normal(size=(T, V, 3)).astype(np.float32) * [0.5, 0.1, 0.1] + [0, 0, 6.0]).float().cuda()
    kp = torch.from_numpy(rng.uniform(100, 500, (T, V, J, 2)).astype(np.float32)).cuda()
    conf = torch.rand(T, V, J).cuda()
    geometry.triangulate_triage(K, R, t, kp, conf)
    geometry.triangulate_joints(K, R, t, kp)
    if args.kernel_only:
        for _ in range(args.reps):
            geometry.triangulate_triage(K, R, t, kp, conf)
            geometry.triangulate_joints(K, R, t, kp)
        torch.cuda.synchronize()
        return
    tri = [event_ms(lambda: geometry.triangulate_triage(K, R, t, kp, conf)) for _ in range(args.reps)]
    dlt = [event_ms(lambda: geometry.triangulate_joints(K, R, t, kp)) for _ in range(args.reps)]
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
           "triage_call_ms_median_T4_J17": float(np.median(tri)), "plain_dlt_call_ms_median_T4_J17": float(np.median(dlt)),
           "note": "device_call = HIP events around geometry.person_origin (allocation + launch + kernel); host = the stage "
                   "it replaces: Tensor.cpu().numpy() of the maps, then extract_person_points + mean per map (host timer)"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
