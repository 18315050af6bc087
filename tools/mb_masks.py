"""Call times of the mask analysis (csrc/masks.hip) at the front camera's own sizes.

    python tools/mb_masks.py [--frames 243] [--reps 5] [--json out.json]

Components, the distance transform, the inner point and boxes on a 243-frame 1920 x 1080 clip of one person mask a frame
(a body-sized blob of ellipses with a few holes and some hundred sprinkles, built on the device); IoU and NMS on 200 x 200
masks of 288 x 288 (SAM3's low-resolution masks).  Beside mask_boxes and mask_iou the same results by the torch-op
formulation the reference uses (row / column any-reductions and index extremes; an [N, M, H W] boolean AND / OR summed over the
pixels), on the same device, checked equal first.  Every figure is a call through the Python wrapper (output and workspace
allocation included), HIP events around `reps` back-to-back calls after two warm-up calls, the median of five such timings
(minimum and maximum beside it)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from skiing_analysis_pytorch_amd import geometry  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(fn, reps, rounds=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn, reps) for _ in range(rounds)]
    return dict(ms=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)))


def person_clip(F, H, W, seed=0):
    """bool [F, H, W] on the device: a figure about 400 pixels tall that wanders over the frame, with holes and sprinkles"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys = torch.arange(H, device="cuda", dtype=torch.float32)[None, :, None]
    xs = torch.arange(W, device="cuda", dtype=torch.float32)[None, None, :]
    t = torch.linspace(0, 1, F, device="cuda")[:, None, None]
    cx, cy = W * (0.2 + 0.6 * t), H * (0.5 + 0.2 * torch.sin(6 * t))
    m = torch.zeros((F, H, W), dtype=torch.bool, device="cuda")
    for dx, dy, rx, ry in ((0, -150, 35, 40), (0, -40, 60, 90), (-35, 110, 25, 90), (35, 110, 25, 90), (-90, -60, 45, 18), (90, -60, 45, 18)):
        m |= ((xs - cx - dx) / rx) ** 2 + ((ys - cy - dy) / ry) ** 2 <= 1.0
    noise = torch.rand((F, H, W), device="cuda", generator=g)
    return (m & (noise > 2e-4)) | (noise < 1e-4)


def boxes_by_torch_ops(masks):
    """the reference's formulation of masks_to_boxes: which rows and columns hold a pixel, then the extremes of their indices"""
    N, H, W = masks.shape
    cols, rows = masks.any(dim=1), masks.any(dim=2)
    x, y = torch.arange(W, device=masks.device), torch.arange(H, device=masks.device)
    return torch.stack([torch.where(cols, x, W).amin(1), torch.where(rows, y, H).amin(1), torch.where(cols, x, 0).amax(1),
                        torch.where(rows, y, 0).amax(1)], dim=1)


def iou_by_torch_ops(a, b):
    """the reference's formulation of mask_iou: the [N, M, H W] AND and OR, summed over the pixels"""
    fa, fb = a.flatten(1)[:, None], b.flatten(1)[None]
    inter, union = (fa & fb).sum(2).float(), (fa | fb).sum(2).float()
    return inter / union.clamp(min=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=243)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    F, H, W = a.frames, 1080, 1920
    clip = person_clip(F, H, W)
    rows = []

    def row(name, fn, **extra):
        r = dict(call=name, **measure(fn, a.reps), **extra)
        rows.append(r)
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()), flush=True)

    comp = geometry.mask_components(clip, 8, 256)
    shape = dict(masks=F, H=H, W=W, foreground=float(clip.float().mean()), components_mean=float(comp.count.float().mean()))
    del comp
    row("mask_components(8, max_components=256)", lambda: geometry.mask_components(clip, 8, 256), **shape)
    row("mask_components(8, max_components=0)", lambda: geometry.mask_components(clip, 8, 0), **shape)
    row("mask_components(4, max_components=0)", lambda: geometry.mask_components(clip, 4, 0), **shape)
    row("distance_transform(border_zero=False)", lambda: geometry.distance_transform(clip), **shape)
    row("mask_inner_point(border_zero=True)", lambda: geometry.mask_inner_point(clip), **shape)
    assert torch.equal(geometry.mask_boxes(clip).xyxy.long(), boxes_by_torch_ops(clip))
    row("mask_boxes", lambda: geometry.mask_boxes(clip), **shape)
    row("boxes by torch ops", lambda: boxes_by_torch_ops(clip), **shape)
    row("clip.clone() (the mask bytes, once in and once out)", lambda: clip.clone(), **shape)
    del clip
    torch.cuda.empty_cache()

    N, h, w = 200, 288, 288
    g = torch.Generator(device="cuda").manual_seed(1)
    yy = torch.arange(h, device="cuda")[None, :, None]
    xx = torch.arange(w, device="cuda")[None, None, :]
    c = torch.randint(40, 248, (N, 2), device="cuda", generator=g)
    r = torch.randint(10, 60, (N, 2), device="cuda", generator=g)
    low = ((xx - c[:, 0, None, None]).abs() <= r[:, 0, None, None]) & ((yy - c[:, 1, None, None]).abs() <= r[:, 1, None, None])
    shape = dict(N=N, M=N, H=h, W=w)
    got = geometry.mask_iou(low, low)
    assert torch.equal(got.iou, iou_by_torch_ops(low, low))
    row("mask_iou", lambda: geometry.mask_iou(low, low), **shape)
    row("iou by torch ops", lambda: iou_by_torch_ops(low, low), **shape)
    scores = torch.rand(N, device="cuda", generator=g)
    row("nms_greedy", lambda: geometry.nms_greedy(got.iou, scores, 0.5), N=N, kept=int(geometry.nms_greedy(got.iou, scores, 0.5).sum()))
    big = torch.rand((1024, 1024), device="cuda", generator=g)
    big = torch.where(big > 0.98, big, torch.zeros_like(big))
    s1024 = torch.rand(1024, device="cuda", generator=g)
    row("nms_greedy", lambda: geometry.nms_greedy(big, s1024, 0.5), N=1024, kept=int(geometry.nms_greedy(big, s1024, 0.5).sum()))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
