"""Call times of the lens kernels (csrc/lens.hip) on the rig's calibration (tests/golden/calibration.npz).

    python tools/mb_lens.py [--reps 200] [--json out.json]

HIP events around `reps` back-to-back calls after three warm-up calls, the median of five such rounds; once for the
wrappers (preprocess.undistort_images, geometry.undistort_points: their output allocations included) and once for the
library calls alone on preallocated buffers.  Frames: uint8 RGB 1080 x 1920, one frame, two cameras x four frames (the
entry point's call at steps_per_call = 4) and a grey frame; the achieved bandwidth counts the algorithmic bytes only, one
read of the source and one write of the result (2 H W ch a frame), against --peak-gbs (default 8000, the MI355X's HBM3E).
Points: 17 joints x 243 frames x 2 views and 1e6 points, 20 and 5 iterations.  Also prints how many values of the frame
differ from the restatement's (tests/lens_restated.py)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import lens_restated as lr  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, formats, geometry, preprocess  # noqa: E402


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
    return float(np.median(rounds)), float(min(rounds)), float(max(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--peak-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cal = formats.load_calibration(Path(__file__).resolve().parent.parent / "tests" / "golden" / "calibration.npz")
    K, d = cal.K, cal.dist
    d12 = geometry.lens_coeffs(d)
    lib, st = _lib.lib(), _lib.current_stream()
    rng = np.random.default_rng(0)
    rows = []
    for C, F, ch in ((1, 1, 3), (2, 4, 3), (1, 1, 1)):
        H, W = 1080, 1920
        src = torch.from_numpy(rng.integers(0, 256, (C, F, H, W, ch), dtype=np.uint8)).cuda()
        out = torch.empty_like(src)
        Kc = np.ascontiguousarray(np.broadcast_to(K, (C, 3, 3)))
        dc = np.ascontiguousarray(np.broadcast_to(d12, (C, 12)))

        def raw():
            _lib.check(lib.skimi_undistort_u8(src.data_ptr(), out.data_ptr(), Kc.ctypes.data, dc.ctypes.data, None, C, F, H, W, H, W, ch, st),
                       "skimi_undistort_u8")

        med, lo, hi = device_ms(raw, a.reps)
        wmed, _, _ = device_ms(lambda: preprocess.undistort_images(src, Kc, dc), a.reps)
        nbytes = 2.0 * C * F * H * W * ch
        row = dict(call="undistort_u8", C=C, F=F, H=H, W=W, ch=ch, library_ms=med, library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed,
                   algorithmic_MB=nbytes / 1e6, achieved_GBs=nbytes / (med * 1e-3) / 1e9, share_of_peak=nbytes / (med * 1e-3) / 1e9 / a.peak_gbs)
        if (C, F, ch) == (1, 1, 3):
            want = lr.undistort_image(src[0, 0].cpu().numpy(), K, d)
            raw()
            row["values_differing_from_restatement"] = int((out[0, 0].cpu().numpy() != want).sum())
        rows.append(row)
    for n, outer, V in ((17, 243, 2), (1_000_000, 1, 1)):
        x = torch.from_numpy(rng.uniform([0, 0], [1920, 1080], (outer, V, n, 2))).cuda()
        o, r = torch.empty_like(x), torch.empty(x.shape[:-1], dtype=torch.float64, device="cuda")
        Kc = np.ascontiguousarray(np.broadcast_to(K, (V, 3, 3)))
        dc = np.ascontiguousarray(np.broadcast_to(d12, (V, 12)))
        for iters in (20, 5):
            def raw():
                _lib.check(lib.skimi_undistort_points(x.data_ptr(), Kc.ctypes.data, dc.ctypes.data, None, None, outer, V, n, iters, 0,
                                                      o.data_ptr(), r.data_ptr(), st), "skimi_undistort_points")

            med, lo, hi = device_ms(raw, a.reps)
            wmed, _, _ = device_ms(lambda: geometry.undistort_points(x, Kc, dc, iters=iters), a.reps)
            rows.append(dict(call="undistort_points", points=outer * V * n, iters=iters, library_ms=med, library_ms_min=lo, library_ms_max=hi,
                             wrapper_ms=wmed))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows, peak_gbs=a.peak_gbs), indent=1))


if __name__ == "__main__":
    main()
