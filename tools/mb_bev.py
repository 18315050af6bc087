"""Call times of the bird's-eye-view kernels (csrc/bev.hip).

    python tools/mb_bev.py [--reps 100] [--json out.json]

The perspective warp (skimi_warp_perspective_u8) at 1080 x 1920 x 3 -> 1600 x 800 x 3 (the reference's default plan), T = 1
and T = 64 frames, INTERLEAVED in one process with the lens warp (skimi_undistort_u8, the rig's calibration of
tests/golden/calibration.npz) at the same input and output shapes: the same traffic, more arithmetic per pixel.  Two
geometries: `affine`, a scaling of the plan onto the frame with a trace of perspective (a wave's gathers stay in two source
rows, as the lens warp's), and `slope`, the reference's default ground points (the far rows of the plan gather sparsely
from a few source rows; recorded, not compared).  HIP events around `reps` back-to-back library calls on preallocated
buffers after three warm-up calls; a round times lens, warp, lens, warp and the figure is the median of five rounds; then
the same pair through the Python wrappers (preprocess.undistort_images, preprocess.warp_perspective: argument checks and
the output allocation included), which is what a caller sees.  The
achieved bandwidth counts the algorithmic bytes (one read of the source, one write of the plan) against --peak-gbs.

Then the small calls: the fit at n = 4, 64 and 1100 (G = 1 and G = 64), points at 17 x 243, the skeleton at T = 243, J = 21
and the track at P = 2, T = 243; and how many bytes of a warped frame differ from the restatement's."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bev_cases as bc  # noqa: E402
import bev_restated as br  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, formats, geometry, preprocess  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def interleaved(fns, reps, rounds=5):
    """-> per function (median, min, max) ms over `rounds` rounds that time every function twice in turn"""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for _ in range(2):
            for k, fn in enumerate(fns):
                times[k].append(timed(fn, reps))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--peak-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, st = _lib.lib(), _lib.current_stream()
    cal = formats.load_calibration(ROOT / "tests" / "golden" / "calibration.npz")
    K = np.ascontiguousarray(cal.K.reshape(1, 3, 3))
    d12 = np.ascontiguousarray(geometry.lens_coeffs(cal.dist).reshape(1, 12))
    H, W, OH, OW, ch = 1080, 1920, 1600, 800, 3
    (bw, bh), S = br.make_bev_canvas()
    assert (bw, bh) == (OW, OH)
    slope = br.homography_fit(bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M, S)["Hinv"]
    affine = np.array([[W / OW, 0.0, 0.0], [0.0, H / OH, 0.0], [1e-5, 2e-5, 1.0]])
    rng = np.random.default_rng(0)
    rows = []
    for T in (1, 64):
        reps = a.reps if T == 1 else max(a.reps // 10, 5)
        src = torch.from_numpy(rng.integers(0, 256, (1, T, H, W, ch), dtype=np.uint8)).cuda()
        out_w, out_l = (torch.empty((1, T, OH, OW, ch), dtype=torch.uint8, device="cuda") for _ in range(2))
        new_K = np.ascontiguousarray((np.diag([OW / W, OH / H, 1.0]) @ K[0]).reshape(1, 3, 3))   # the whole frame, at the plan's size

        def lens():
            _lib.check(lib.skimi_undistort_u8(src.data_ptr(), out_l.data_ptr(), K.ctypes.data, d12.ctypes.data, new_K.ctypes.data, 1, T, H, W,
                                              OH, OW, ch, st), "skimi_undistort_u8")

        nbytes = float(T) * (H * W + OH * OW) * ch
        for name, G in (("affine", affine), ("slope", slope)):
            g = torch.from_numpy(np.ascontiguousarray(G.reshape(1, 9))).cuda()

            def warp():
                _lib.check(lib.skimi_warp_perspective_u8(src.data_ptr(), out_w.data_ptr(), g.data_ptr(), 0, 1, T, H, W, OH, OW, ch, st),
                           "skimi_warp_perspective_u8")

            (lm, llo, lhi), (wm, wlo, whi) = interleaved((lens, warp), reps)
            # the same pair as a caller of the Python wrappers sees it: argument checks and the output allocation included
            g33 = g.view(3, 3)
            (lwm, _, _), (wwm, _, _) = interleaved((lambda: preprocess.undistort_images(src[0], K[0], d12[0], new_K=new_K[0], out_size=(OW, OH)),
                                                    lambda: preprocess.warp_perspective(src[0], g33, (OW, OH))), reps)
            row = dict(call="warp_perspective_u8", geometry=name, T=T, reps=reps, warp_ms=wm, warp_ms_min=wlo, warp_ms_max=whi, lens_ms=lm,
                       lens_ms_min=llo, lens_ms_max=lhi, warp_over_lens=wm / lm, warp_wrapper_ms=wwm, lens_wrapper_ms=lwm,
                       wrapper_warp_over_lens=wwm / lwm, algorithmic_MB=nbytes / 1e6,
                       warp_GBs=nbytes / (wm * 1e-3) / 1e9, warp_share_of_peak=nbytes / (wm * 1e-3) / 1e9 / a.peak_gbs)
            if T == 1:
                warp()
                values = br.warp_values(src[0, 0].cpu().numpy(), G, (OW, OH))
                got = out_w[0, 0].cpu().numpy()
                row["near_tie_bytes"] = int(br.near_tie(values).sum())
                row["bytes_differing_from_restatement"] = int((got != np.floor(values + 0.5).astype(np.uint8)).sum())
                row["frame_bytes"] = int(got.size)
            rows.append(row)

    def small(call, fn, **info):
        fn()
        torch.cuda.synchronize()
        t = [timed(fn, a.reps) for _ in range(5)]
        rows.append(dict(call=call, **info, wrapper_ms=float(np.median(t)), wrapper_ms_min=float(min(t)), wrapper_ms_max=float(max(t))))

    for n in (4, 64, 1100):
        for G in (1, 64):
            s, d = (bc.DEFAULT_IMG_PTS, bc.DEFAULT_BEV_PTS_M) if n == 4 else bc.noisy_fit(n)
            sd, dd = (torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x, (G, n, 2)))).cuda() for x in (s, d))
            small("homography_fit", lambda: geometry.homography_fit(sd, dd, post=S), n=n, G=G)
    x, Hs = bc.points_case(17 * 243, G=1)
    xd, Hd = torch.from_numpy(x[0]).cuda(), torch.from_numpy(Hs[0]).cuda()
    small("homography_points", lambda: geometry.homography_points(xd, Hd), points=17 * 243)
    X, cpx = bc.skeleton_case(243, 21)
    Xd, cd = torch.from_numpy(X).cuda(), torch.from_numpy(cpx).cuda()
    small("bev_skeleton", lambda: geometry.bev_skeleton(Xd, cd, 0.02, (0, 2), True), T=243, J=21)
    pd = torch.from_numpy(bc.track_case(2, 243)).cuda()
    small("ground_track", lambda: geometry.ground_track(pd, 30.0), P=2, T=243)

    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows, peak_gbs=a.peak_gbs), indent=1))


if __name__ == "__main__":
    main()
