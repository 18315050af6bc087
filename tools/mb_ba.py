"""Bundle adjustment (csrc/ba.hip, geometry.bundle_adjust) against its yardstick: the float64 restatement of
tests/ba_restated.py run by torch on the GPU (an autograd graph + Adam per iteration, one mode per run), interleaved.

For each T in {64, 512, 4096} (C = 2, J = 17) the HIP launch runs the three modes in ONE launch at 200 and 10,000
iterations.  The yardstick runs the three modes one after the other at a reduced iteration count (--yard-iters) and its
time is scaled linearly to 200 and 10,000 iterations; the JSON says so.

    python tools/mb_ba.py [--reps 3] [--yard-iters 20] [--out result.json]

One JSON object is printed (and written with --out); profiles/ba.md records a run.
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
import torch  # noqa: E402

MODES = ("pose_only", "pose_cam_t", "full")


def clip(T, C=2, J=17, seed=0):
    rng = np.random.default_rng(seed)
    K = np.zeros((C, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = 1000.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 960.0, 540.0, 1.0
    R, t = np.zeros((T, C, 3, 3)), np.zeros((T, C, 3))
    for c in range(C):
        a = 2 * np.pi * c / C + 0.3
        ctr = np.array([4 * np.sin(a), -0.3, -4 * np.cos(a)])
        z = -ctr / np.linalg.norm(ctr)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R[:, c] = np.stack([x, np.cross(z, x), z])
        t[:, c] = -R[0, c] @ ctr + rng.normal(0, 0.02, (T, 3))
    X = rng.normal(0, 0.4, (J, 3)) + np.cumsum(rng.normal(0, 0.01, (T, J, 3)), 0)
    Xc = np.einsum("tcij,tkj->tcki", R, X) + t[:, :, None]
    x2d = np.einsum("cij,tckj->tcki", K, Xc / Xc[..., 2:3])[..., :2] + rng.normal(0, 2.0, (T, C, J, 2))
    conf = rng.uniform(0.3, 1.0, (T, C, J))
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(a).to(dev) for a in (K, R, t, X + rng.normal(0, 0.02, X.shape), x2d, conf)]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yard-iters", type=int, default=20)
    ap.add_argument("--Ts", default="64,512,4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ba_restated as ref
    from skiing_analysis_pytorch_amd import geometry

    rows = []
    for T in [int(v) for v in args.Ts.split(",")]:
        c = clip(T)
        per = int(geometry.lib().skimi_ba_workspace_bytes(T, 2, 17, 1))
        geometry.bundle_adjust(*c, modes=MODES, num_iters=5)          # warm-up (code object, LDS opt-in)
        ref.run(*c, mode="full", num_iters=2, device=c[0].device)
        hip = {200: [], 10000: []}
        yard = []
        for _ in range(args.reps):        # interleaved: HIP 200, yardstick, HIP 10000
            hip[200].append(event_ms(lambda: geometry.bundle_adjust(*c, modes=MODES, num_iters=200, lr=1e-2)))
            yard.append(event_ms(lambda: [ref.run(*c, mode=m, num_iters=args.yard_iters, lr=1e-2, device=c[0].device)
                                          for m in MODES]))
            hip[10000].append(event_ms(lambda: geometry.bundle_adjust(*c, modes=MODES, num_iters=10000, lr=1e-2)))
        y_it = float(np.median(yard)) / args.yard_iters
        row = {"T": T, "C": 2, "J": 17, "modes": 3, "state_bytes_per_mode": per,
               "placement": "lds" if per <= 160 * 1024 - 4096 else "workspace",
               "hip_ms_200": float(np.median(hip[200])), "hip_ms_10000": float(np.median(hip[10000])),
               "yardstick_ms_per_iter_3_modes": y_it,
               "yardstick_ms_200_scaled": y_it * 200, "yardstick_ms_10000_scaled": y_it * 10000,
               "yardstick_iters_run": args.yard_iters}
        row["speedup_200"] = row["yardstick_ms_200_scaled"] / row["hip_ms_200"]
        row["speedup_10000"] = row["yardstick_ms_10000_scaled"] / row["hip_ms_10000"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "note": f"yardstick = tests/ba_restated.py run by torch on the GPU in float64, {args.yard_iters} iterations "
                   "per mode, three modes in turn, time scaled linearly to 200 / 10000 iterations; HIP = one launch of "
                   "all three modes at the full iteration count; medians of interleaved repetitions (HIP events)",
           "rows": rows}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
