"""Call times of the rasteriser (csrc/draw.hip) beside a copy of the same clip.

    python tools/mb_draw.py [--frames 243] [--reps 10] [--json out.json]

A 243-frame 1920 x 1080 x 3 clip with draw_keypoints' list for one 17-joint skeleton per frame (17 discs, 34 label places,
16 edges: 67 records a frame), drawn out of place into a preallocated clip (skimi_draw_shapes_u8) and in place, INTERLEAVED
in one process with frames.clone() of the same clip on the same device: the clone moves the bytes the out-of-place draw
moves and is the yardstick.  HIP events around `reps` back-to-back calls after three warm-up calls; a round times clone,
out of place, in place, each twice in turn, and the figure is the median of five rounds (min and max beside it).  Then
the same through the Python wrapper (draw.draw_keypoints: the builders' torch ops and the output allocation included),
which is what a caller sees; the share of 64 x 16 tiles that hold any shape (the rule of include/skimi.h, restated here);
and a 1080p clip whose skeleton is 4 times larger, where more tiles hold shapes.  The clip is larger than the last-level
cache (1.5 GB against 256 MiB), so every call streams from and to HBM."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from skiing_analysis_pytorch_amd import _lib, draw, geometry  # noqa: E402

TILE_W, TILE_H = 64, 16


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


def skeleton_clip(F, H, W, size, seed=0):
    """[F, 17, 2] pixels: a figure about `size` pixels tall that wanders over the frame"""
    rng = np.random.default_rng(seed)
    pose = np.array([[0, -0.46], [-0.02, -0.48], [0.02, -0.48], [-0.05, -0.46], [0.05, -0.46], [-0.12, -0.32], [0.12, -0.32], [-0.18, -0.14],
                     [0.18, -0.14], [-0.2, 0.02], [0.2, 0.02], [-0.08, 0.02], [0.08, 0.02], [-0.1, 0.26], [0.1, 0.26], [-0.1, 0.5], [0.1, 0.5]])
    t = np.linspace(0, 1, F)[:, None]
    centre = np.concatenate([W * (0.2 + 0.6 * t), H * (0.5 + 0.2 * np.sin(6 * t))], axis=1)
    return centre[:, None, :] + size * pose[None] + rng.normal(0, 1.0, (F, 17, 2))


def tile_share(shapes, H, W):
    """the share of (frame, tile) pairs whose list is not empty: the extent grown by the radius (ring: r + h) plus one pixel"""
    s = shapes.astype(np.int64)
    F = s.shape[0]
    nx, ny = -(-W // TILE_W), -(-H // TILE_H)
    hit = np.zeros((F, ny, nx), dtype=bool)
    for f in range(F):
        for kind, x0, y0, x1, y1, r, _, opacity in s[f]:
            if kind < 1 or kind > 4 or opacity <= 0:
                continue
            if kind == 4:
                lo_x, lo_y = (x0 >> 4) * 16, (y0 >> 4) * 16
                hi_x, hi_y, g = lo_x + 16 * (5 * max(r, 1) - 1), lo_y + 16 * (7 * max(r, 1) - 1), 16
            else:
                g = r + 16 + (x1 if kind == 2 else 0)
                lo_x, hi_x, lo_y, hi_y = (min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)) if kind == 3 else (x0, x0, y0, y0)
            tx = np.arange(nx) * TILE_W * 16
            ty = np.arange(ny) * TILE_H * 16
            tx1 = (np.minimum(np.arange(nx) * TILE_W + TILE_W, W) - 1) * 16
            ty1 = (np.minimum(np.arange(ny) * TILE_H + TILE_H, H) - 1) * 16
            mx = (lo_x - g <= tx1) & (hi_x + g >= tx)
            my = (lo_y - g <= ty1) & (hi_y + g >= ty)
            hit[f] |= my[:, None] & mx[None, :]
    return float(hit.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--peak-gbs", type=float, default=8000.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lib, st = _lib.lib(), _lib.current_stream()
    F, H, W, ch = a.frames, 1080, 1920, 3
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (F, H, W, ch), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty_like(frames)
    work = frames.clone()
    font = torch.from_numpy(geometry.font_5x7()).cuda()
    nbytes = 2.0 * frames.numel()
    rows = []
    for name, size in (("skeleton_300px", 300.0), ("skeleton_1200px", 1200.0)):
        kp = torch.from_numpy(skeleton_clip(F, H, W, size)).cuda()
        shapes = draw.keypoint_shapes(kp).contiguous()
        P = int(shapes.shape[1])

        def draw_to(dst):
            _lib.check(lib.skimi_draw_shapes_u8(frames.data_ptr() if dst is out else dst.data_ptr(), dst.data_ptr(), shapes.data_ptr(), 3,
                                                font.data_ptr(), 1, F, H, W, ch, P, st), "skimi_draw_shapes_u8")

        (cm, clo, chi), (om, olo, ohi), (im, ilo, ihi) = interleaved((lambda: frames.clone(), lambda: draw_to(out), lambda: draw_to(work)), a.reps)
        (wcm, _, _), (wom, _, _) = interleaved((lambda: frames.clone(), lambda: draw.draw_keypoints(frames, kp)), a.reps)
        draw_to(out)
        changed = float((out != frames).any(dim=-1).float().mean())
        rows.append(dict(case=name, frames=F, H=H, W=W, ch=ch, records_per_frame=P, reps=a.reps, clone_ms=cm, clone_ms_min=clo, clone_ms_max=chi,
                         draw_out_of_place_ms=om, draw_out_of_place_ms_min=olo, draw_out_of_place_ms_max=ohi, draw_in_place_ms=im,
                         draw_in_place_ms_min=ilo, draw_in_place_ms_max=ihi, out_of_place_over_clone=om / cm, in_place_over_clone=im / cm,
                         wrapper_draw_keypoints_ms=wom, wrapper_clone_ms=wcm, wrapper_over_clone=wom / wcm,
                         tiles_with_shapes=tile_share(shapes.cpu().numpy(), H, W), pixels_changed=changed, algorithmic_MB=nbytes / 1e6,
                         clone_GBs=nbytes / (cm * 1e-3) / 1e9, draw_out_of_place_GBs=nbytes / (om * 1e-3) / 1e9,
                         draw_share_of_peak=nbytes / (om * 1e-3) / 1e9 / a.peak_gbs))
    for row in rows:
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in row.items()), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows, peak_gbs=a.peak_gbs), indent=1))


if __name__ == "__main__":
    main()
