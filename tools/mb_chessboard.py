"""Call times of the chessboard detector (csrc/chessboard.hip) on 24 frames of 1920 x 1080 x 3, the reference's calibration set.

    python tools/mb_chessboard.py [--reps 20] [--json out.json] [--no-cpu]

The frames are the rendered boards of tests/chessboard_cases.py (views 0, 9, 13 in turn) enlarged three times by pixel
repetition, with differing colour channels.  HIP events around `reps` back-to-back calls after three warm-up calls, the
median of five such rounds (minimum and maximum beside it): the library calls on preallocated buffers, the two wrappers, and
calibration.find_chessboard_corners with its read-back and host ordering (a host clock around it, which ends in the
read-back's synchronise).  The response launch's own time comes from a kernel trace (rocprofv3 --kernel-trace --stats --
python tools/mb_chessboard.py --reps 5 --no-cpu), not from here; its algorithmic bytes are printed: one read of the frames
and one write of the int32 response (the gray plane is not stored).  --no-cpu skips the restatement's time on one frame."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import chessboard_cases as cb  # noqa: E402
import chessboard_restated as cs  # noqa: E402
from skiing_analysis_pytorch_amd import _lib, calibration, geometry  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    big = [cb.channels(np.repeat(np.repeat(cb.render(v), 3, axis=0), 3, axis=1), 3) for v in cb.VIEWS]
    host = np.stack([big[i % len(big)] for i in range(a.frames)])
    N, H, W, ch = host.shape
    frames = torch.from_numpy(host).cuda()
    lib, st = _lib.lib(), _lib.current_stream()
    M = 1024
    xy, resp = torch.empty((N, M, 2), dtype=torch.int32, device="cuda"), torch.empty((N, M), dtype=torch.int32, device="cuda")
    count, rmax = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
    nws = int(lib.skimi_chess_workspace_bytes(N, H, W))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def raw_candidates():
        _lib.check(lib.skimi_chess_candidates(frames.data_ptr(), N, H, W, ch, 38, 4, M, xy.data_ptr(), resp.data_ptr(), count.data_ptr(),
                                              rmax.data_ptr(), ws.data_ptr(), nws, st), "skimi_chess_candidates")

    raw_candidates()
    pts = xy.double()
    out, ok = torch.empty_like(pts), torch.empty((N, M), dtype=torch.uint8, device="cuda")
    rows = [dict(frames=N, H=H, W=W, ch=ch, workspace_MB=nws / 1e6, candidates=count.cpu().tolist(),
                 response_algorithmic_MB=(N * H * W * ch + 4.0 * N * H * W) / 1e6)]
    med, lo, hi = device_ms(raw_candidates, a.reps)
    wmed, _, _ = device_ms(lambda: geometry.chessboard_candidates(frames), a.reps)
    rows.append(dict(call="skimi_chess_candidates", library_ms=med, library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed))
    for win in ((5, 5), (11, 11)):
        def raw_subpix():
            _lib.check(lib.skimi_corner_subpix(frames.data_ptr(), N, H, W, ch, pts.data_ptr(), count.data_ptr(), M, win[0], win[1], 30,
                                               out.data_ptr(), ok.data_ptr(), st), "skimi_corner_subpix")

        med, lo, hi = device_ms(raw_subpix, a.reps)
        wmed, _, _ = device_ms(lambda: geometry.corner_subpix(frames, pts, count, win=win), a.reps)
        rows.append(dict(call="skimi_corner_subpix", win=list(win), points=int(count.clamp(max=M).sum()), library_ms=med,
                         library_ms_min=lo, library_ms_max=hi, wrapper_ms=wmed))
    for win in ((5, 5), (11, 11)):
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, found = calibration.find_chessboard_corners(frames, cb.BOARD, win=win)
            times.append((time.perf_counter() - t) * 1e3)
        rows.append(dict(call="find_chessboard_corners", win=list(win), found=int(found.sum()), host_ms=float(np.median(times)),
                         host_ms_min=float(min(times)), host_ms_max=float(max(times))))
    if not a.no_cpu:
        t = time.perf_counter()
        board = cs.find_chessboard_corners(host[0], cb.BOARD, win=(11, 11))[0]
        rows.append(dict(call="restatement, one frame (NumPy)", found=board is not None, host_ms=(time.perf_counter() - t) * 1e3))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
