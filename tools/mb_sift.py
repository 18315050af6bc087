"""Call times of the SIFT-style features and the L2 matcher (csrc/sift.hip) on two clips of 1920 x 1080 x 3 frames.

    python tools/mb_sift.py [--frames 8] [--reps 10] [--json out.json] [--no-cpu]

The frames are those of tools/mb_features.py: the view pairs of tests/features_cases.py enlarged three times by pixel
repetition and tiled 2 x 2, cut to 1080 rows, with differing colour channels.  HIP events around `reps` back-to-back calls
after three warm-up calls, the median of five such rounds (minimum and maximum beside it): skimi_sift_features on one clip
with preallocated buffers (3000 features, the default octaves), skimi_match_l2 on the clip pair's descriptor sets (ratio
0.75, 1000 matches; and with the cross check, which runs the second direction), the two wrappers, and
camera_position.estimate_camera_poses_from_SIFT with its read-back (a host clock).  The per-kernel times come from a kernel
trace (rocprofv3 --kernel-trace --stats -- python tools/mb_sift.py --reps 3 --no-cpu), not from here; the blur launches'
algorithmic bytes are printed: one read of the source layer (the frame's bytes for the first) and one write of the layer.
--no-cpu skips the restatement's time on one frame and one pair of sets."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import features_cases as fc  # noqa: E402
import sift_restated as sr  # noqa: E402
from mb_features import device_ms, enlarge  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, camera_position, geometry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    pairs = [fc.view_pair(p[0], s) for s in (0, 1) for p in fc.PAIRS]
    host = [np.stack([enlarge(pairs[i % len(pairs)][v], 10 * v + i) for i in range(a.frames)]) for v in (0, 1)]
    N, H, W, ch = host[0].shape
    clips = [torch.from_numpy(h).cuda() for h in host]
    lib, st = _lib.lib(), _lib.current_stream()
    M, O, mm = 3000, geometry.sift_octaves(H, W), 1000
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")   # noqa: E731
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device="cuda")   # noqa: E731
    xy, xyl, octv, lay, sig, resp, ang = f64(N, M, 2), i32(N, M, 2), i32(N, M), i32(N, M), f64(N, M), f64(N, M), f64(N, M)
    desc, count, ocount = torch.empty((N, M, 128), dtype=torch.uint8, device="cuda"), i32(N), i32(N, O)
    nws = int(lib.skimi_sift_workspace_bytes(N, H, W, O))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    taps = torch.from_numpy(geometry.sift_taps()).cuda()

    def raw_features():
        _lib.check(lib.skimi_sift_features(clips[0].data_ptr(), N, H, W, ch, O, M, None, taps.data_ptr(), xy.data_ptr(), xyl.data_ptr(),
                                           octv.data_ptr(), lay.data_ptr(), sig.data_ptr(), resp.data_ptr(), ang.data_ptr(), desc.data_ptr(),
                                           count.data_ptr(), ocount.data_ptr(), ws.data_ptr(), nws, st), "skimi_sift_features")

    raw_features()
    sizes, w, h = [], W, H
    for _ in range(O):
        sizes.append(w * h)
        w, h = (w + 1) // 2, (h + 1) // 2
    # a blur reads its source layer and writes its layer: 4 + 4 bytes a pixel, ch + 4 for the first; the half launch 1 + 4
    blur_bytes = N * (sizes[0] * (ch + 4) + 5 * 8 * sizes[0] + sum(5 * 8 * s + 5 * s for s in sizes[1:]))
    rows = [dict(frames=N, H=H, W=W, ch=ch, max_features=M, octaves=O, workspace_MB=nws / 1e6, workspace_MB_per_frame=nws / 1e6 / N,
                 keypoints=count.cpu().tolist(), candidates=ocount.sum(dim=1).cpu().tolist(), candidates_octave0=ocount[:, 0].cpu().tolist(),
                 scale_space_launches=6 * O, scale_space_algorithmic_MB=blur_bytes / 1e6,
                 octave0_blur_algorithmic_MB=N * 8 * sizes[0] / 1e6)]
    med, lo, hi = device_ms(raw_features, a.reps)
    wmed, _, _ = device_ms(lambda: geometry.sift_features(clips[0], M), a.reps)
    rows.append(dict(call="skimi_sift_features", library_ms=med, library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed,
                     library_ms_per_frame=med / N))
    fa, fb = geometry.sift_features(clips[0], M), geometry.sift_features(clips[1], M)
    pr, d2, s2, cn = i32(N, mm, 2), i32(N, mm), i32(N, mm), i32(N)
    mws_bytes = 8 * N * 2 * M + 4 * N * M
    mws = torch.empty(mws_bytes, dtype=torch.uint8, device="cuda")
    for cross in (0, 1):
        def raw_match():
            _lib.check(lib.skimi_match_l2(fa.desc.data_ptr(), fa.count.data_ptr(), M, fb.desc.data_ptr(), fb.count.data_ptr(), M, N, cross,
                                          0.75, -1, mm, pr.data_ptr(), d2.data_ptr(), s2.data_ptr(), cn.data_ptr(), mws.data_ptr(), mws_bytes,
                                          st), "skimi_match_l2")

        med, lo, hi = device_ms(raw_match, a.reps)
        wmed, _, _ = device_ms(lambda: geometry.match_l2(fa.desc, fa.count, fb.desc, fb.count, cross_check=bool(cross), max_matches=mm), a.reps)
        rows.append(dict(call="skimi_match_l2", cross_check=cross, sets=N, rows=[fa.count.cpu().tolist(), fb.count.cpu().tolist()],
                         matches=cn.cpu().tolist(), library_ms=med, library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed,
                         library_ms_per_pair=med / N))
    K = fc.K.copy()
    K[:2] *= 6.0
    rgb = [c.flip(-1).contiguous() for c in clips]
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        _, _, _, ok = camera_position.estimate_camera_poses_from_SIFT(rgb[0], rgb[1], K, 0.5)
        times.append((time.perf_counter() - t) * 1e3)
    rows.append(dict(call="estimate_camera_poses_from_SIFT", frames=N, poses=int(ok.sum()), host_ms=float(np.median(times)),
                     host_ms_min=float(min(times)), host_ms_max=float(max(times))))
    if not a.no_cpu:
        t = time.perf_counter()
        one = sr.sift_features(host[0][0], M)
        t1 = time.perf_counter()
        other = sr.sift_features(host[1][0], M)
        t2 = time.perf_counter()
        sr.match_l2(one["desc"][:one["count"]], other["desc"][:other["count"]], 0.75, max_matches=mm)
        rows.append(dict(call="restatement, one frame and one pair of sets (NumPy)", features_host_ms=(t1 - t) * 1e3,
                         match_host_ms=(time.perf_counter() - t2) * 1e3))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
