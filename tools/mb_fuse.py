"""Call times of the device fusion and smoothing next to the host functions on the same inputs:
geometry.fuse_h36m, fuse_views, smooth_ema, smooth_savgol at T = 243 and T = 4096 (J = 17 and 70).

    python tools/mb_fuse.py [--reps 20] [--json out.json]

Device: HIP events around `reps` back-to-back calls of the Python wrapper (allocation of the outputs included), after
three warm-up calls; the median of five such rounds.  Host: wall time of one call of the fuse.py function (the per-frame
Python loop for the two fusions), the median of three."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import fuse_cases as fc  # noqa: E402
from skiing_analysis_pytorch_amd import fuse, geometry  # noqa: E402


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        rounds.append(a.elapsed_time(b) / reps)
    return float(np.median(rounds))


def host_ms(fn):
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    rows = []
    for T in (243, 4096):
        _, L, R = fc._h36m_pair(50, T)
        kw = dict(tau=0.06, allow_scale=False, mirror_right_x=False)
        Ld, Rd = dev(L), dev(R)
        rows.append(dict(call="fuse_h36m", T=T, J=17, device_ms=device_ms(lambda: geometry.fuse_h36m(Ld, Rd, **kw), a.reps),
                         host_ms=host_ms(lambda: fc.host_h36m(L, R, kw))))
        for J, keys in ((17, fc.KEYS17), (70, fc.KEYS70)):
            _, Xl, Xr, Ul, Ur = fc._views_pair(51, T, J)
            vkw = dict(**keys, sigma_px=12.0, sigma_3d=0.08, scale_mode="hip", min_points=8)
            d = [dev(x) for x in (Xl, Xr, Ul, Ur)]
            rows.append(dict(call="fuse_views", T=T, J=J, device_ms=device_ms(lambda: geometry.fuse_views(*d, **vkw), a.reps),
                             host_ms=host_ms(lambda: fc.host_views(Xl, Xr, Ul, Ur, vkw))))
            X = Xl.copy()
            X[np.random.default_rng(52).random(size=(T, J)) < 0.1] = np.nan
            Xd = dev(X)
            rows.append(dict(call="smooth_ema", T=T, J=J, device_ms=device_ms(lambda: geometry.smooth_ema(Xd), a.reps),
                             host_ms=host_ms(lambda: fuse.temporal_smooth_ema(X))))
            rows.append(dict(call="smooth_savgol", T=T, J=J, device_ms=device_ms(lambda: geometry.smooth_savgol(Xd), a.reps),
                             host_ms=host_ms(lambda: fuse.smooth_skeleton(X))))
    for r in rows:
        print(f"{r['call']:14s} T={r['T']:5d} J={r['J']:3d}  device {r['device_ms']:9.4f} ms   host {r['host_ms']:10.3f} ms")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
