"""The scene-cloud call (csrc/scene.hip: ten launches) at the shape a batched VGGT call gives, B = 4 steps of S = 8 views
at 518 x 518, next to the host path it replaces: the device-to-host copy of the dense maps (points, confidences,
images) and the NumPy rules of tests/scene_restated.py (a sort-based percentile per scene, mask, compaction, six more
percentiles).  For context only: nothing here is asserted.

Inputs: points N(0, 2), conf = 1 + exp(N(0, 1)), uniform images, conf_thres 50 (about half the pixels are kept).

    python tools/mb_scene.py [--reps 10] [--batch 4] [--views 8] [--size 518] [--out result.json]

HIP events around the public call (output and workspace allocation + the launches); wall clock around the host path.
Also reported: the device-to-host copy of the kept rows alone, which is what reaches the host with the device path, and
whether the device kept set and scale agree with the host rules on scene 0.
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
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--conf-thres", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import scene_restated as ref
    from skiing_analysis_pytorch_amd import geometry

    B, S, H, W = args.batch, args.views, args.size, args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    points = torch.randn((B, S, H, W, 3), generator=g, device="cuda") * 2.0
    conf = 1.0 + torch.exp(torch.randn((B, S, H, W), generator=g, device="cuda"))
    images = torch.rand((B, S, 3, H, W), generator=g, device="cuda")
    E = torch.eye(3, 4, device="cuda").repeat(B, S, 1, 1) + 0.01 * torch.randn((B, S, 3, 4), generator=g, device="cuda")

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    call = lambda: geometry.scene_point_cloud(points, conf, images, E, conf_thres=args.conf_thres)   # noqa: E731
    for _ in range(3):
        cloud = call()
    torch.cuda.synchronize()
    dev_ms = [event_ms(call) for _ in range(args.reps)]
    counts = cloud.count.cpu().tolist()

    def kept_to_host():
        return [(cloud.xyz[b, :counts[b]].cpu(), cloud.rgb[b, :counts[b]].cpu()) for b in range(B)]

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    kept_ms = [wall_ms(kept_to_host)[0] for _ in range(args.reps)]
    copy_ms, host_ms, agree = [], [], None
    for rep in range(max(1, min(args.reps, 3))):
        ms, (pn, cn, imn, En) = wall_ms(lambda: tuple(a.cpu().numpy() for a in (points, conf, images, E)))
        copy_ms.append(ms)
        t0 = time.perf_counter()
        host = [ref.scene_cloud(pn[b], cn[b], imn[b], En[b], conf_thres=args.conf_thres, align=True) for b in range(B)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
        if agree is None:
            k = counts[0]
            agree = {"count_equal": host[0]["count"] == k,
                     "rgb_equal": bool(np.array_equal(host[0]["rgb"], cloud.rgb[0, :k].cpu().numpy())),
                     "scale_rel_diff": float(abs(host[0]["scale"] - float(cloud.scale[0])) / host[0]["scale"]),
                     "threshold_equal": host[0]["threshold"] == float(cloud.threshold[0])}
    n = S * H * W
    res = {"device": torch.cuda.get_device_name(0), "B": B, "S": S, "H": H, "W": W, "pixels_per_scene": n,
           "conf_thres": args.conf_thres, "launch": geometry.scene_launch(n), "kept": counts, "reps": args.reps,
           "device_call_ms_median": float(np.median(dev_ms)), "device_call_ms_min": float(min(dev_ms)),
           "device_call_ms_max": float(max(dev_ms)), "kept_rows_to_host_ms_median": float(np.median(kept_ms)),
           "dense_maps_to_host_ms_median": float(np.median(copy_ms)), "host_numpy_rules_ms_median": float(np.median(host_ms)),
           "dense_bytes": int(sum(a.numel() * a.element_size() for a in (points, conf, images))),
           "kept_bytes": int(sum(counts) * 15), "agreement_scene0": agree,
           "note": "device call = HIP events around geometry.scene_point_cloud (allocation + ten launches); host = wall clock"}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
