"""Call times of the image features and the Hamming matcher (csrc/features.hip) on two clips of 1920 x 1080 x 3 frames.

    python tools/mb_features.py [--frames 8] [--reps 10] [--json out.json] [--no-cpu]

The frames are the view pairs of tests/features_cases.py enlarged three times by pixel repetition and tiled 2 x 2, cut to
1080 rows, with differing colour channels.  HIP events around `reps` back-to-back calls after three warm-up calls, the median
of five such rounds (minimum and maximum beside it): skimi_orb_features on one clip with preallocated buffers (3000 features,
8 levels, as the reference's cv2.ORB_create(3000)), skimi_match_hamming on the clip pair's descriptor sets (1000 matches),
the two wrappers, and camera_position.estimate_camera_poses_from_ORB with its read-back (a host clock).  The per-kernel
times come from a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/mb_features.py --reps 3 --no-cpu), not from
here; the FAST launch's algorithmic bytes are printed: one read of the gray pyramid and one write of the score map.
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
import features_restated as fr  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, camera_position, geometry  # noqa: E402
from skiing_analysis_pytorch_amd.device import features as df  # noqa: E402


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


def enlarge(gray, seed):
    big = np.tile(np.repeat(np.repeat(gray, 3, axis=0), 3, axis=1), (2, 2))[:1080, :1920]
    return fc.colour(np.ascontiguousarray(big), 3, seed)


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
    M, L, mm = 3000, 8, 1000
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")   # noqa: E731
    xyl, xy, lvl, dirn, score = i32(N, M, 2), torch.empty((N, M, 2), dtype=torch.float64, device="cuda"), i32(N, M), i32(N, M), i32(N, M)
    har, desc, count, lcount = torch.empty((N, M), dtype=torch.int64, device="cuda"), i32(N, M, 8), i32(N), i32(N, L)
    nws = int(lib.skimi_orb_workspace_bytes(N, H, W, L))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    pattern = torch.from_numpy(df.orb_pattern()).cuda()

    def raw_features():
        _lib.check(lib.skimi_orb_features(clips[0].data_ptr(), N, H, W, ch, L, 20, M, None, pattern.data_ptr(), xyl.data_ptr(), xy.data_ptr(),
                                          lvl.data_ptr(), dirn.data_ptr(), score.data_ptr(), har.data_ptr(), desc.data_ptr(),
                                          count.data_ptr(), lcount.data_ptr(), ws.data_ptr(), nws, st), "skimi_orb_features")

    raw_features()
    pyramid = sum(fr.level_size(W, l) * fr.level_size(H, l) for l in range(L))
    rows = [dict(frames=N, H=H, W=W, ch=ch, max_features=M, levels=L, workspace_MB=nws / 1e6, keypoints=count.cpu().tolist(),
                 candidates_level0=lcount[:, 0].cpu().tolist(), pyramid_pixels=pyramid, fast_algorithmic_MB=2.0 * N * pyramid / 1e6)]
    med, lo, hi = device_ms(raw_features, a.reps)
    wmed, _, _ = device_ms(lambda: geometry.orb_features(clips[0], M, L), a.reps)
    rows.append(dict(call="skimi_orb_features", library_ms=med, library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed,
                     library_ms_per_frame=med / N))
    fa, fb = geometry.orb_features(clips[0], M, L), geometry.orb_features(clips[1], M, L)
    pr, di, cn = i32(N, mm, 2), i32(N, mm), i32(N)

    def raw_match():
        _lib.check(lib.skimi_match_hamming(fa.desc.data_ptr(), fa.count.data_ptr(), M, fb.desc.data_ptr(), fb.count.data_ptr(), M, N, 1, -1.0,
                                           -1, mm, pr.data_ptr(), di.data_ptr(), cn.data_ptr(), st), "skimi_match_hamming")

    med, lo, hi = device_ms(raw_match, a.reps)
    wmed, _, _ = device_ms(lambda: geometry.match_hamming(fa.desc, fa.count, fb.desc, fb.count, max_matches=mm), a.reps)
    rows.append(dict(call="skimi_match_hamming", sets=N, matches=cn.cpu().tolist(), library_ms=med, library_ms_min=lo, library_ms_max=hi,
                     wrapper_ms=wmed, library_ms_per_pair=med / N))
    K = fc.K.copy()
    K[:2] *= 6.0
    rgb = [c.flip(-1).contiguous() for c in clips]
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        _, _, _, ok = camera_position.estimate_camera_poses_from_ORB(rgb[0], rgb[1], K, 0.5)
        times.append((time.perf_counter() - t) * 1e3)
    rows.append(dict(call="estimate_camera_poses_from_ORB", frames=N, poses=int(ok.sum()), host_ms=float(np.median(times)),
                     host_ms_min=float(min(times)), host_ms_max=float(max(times))))
    if not a.no_cpu:
        t = time.perf_counter()
        one = fr.orb_features(host[0][0], M, L)
        t1 = time.perf_counter()
        other = fr.orb_features(host[1][0], M, L)
        t2 = time.perf_counter()
        fr.match_hamming(one["desc"][:one["count"]], other["desc"][:other["count"]], max_matches=mm)
        rows.append(dict(call="restatement, one frame and one pair of sets (NumPy)", features_host_ms=(t1 - t) * 1e3,
                         match_host_ms=(time.perf_counter() - t2) * 1e3))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
