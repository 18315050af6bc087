"""Call times of linear assignment, det-track association and the box tracker (csrc/assign.hip) at the front camera's sizes.

    python tools/mb_assign.py [--reps 5] [--json out.json]

linear_assignment at [243, 8, 8], [243, 64, 64] and [1, 1024, 1024] (1 - IoU-like costs: uniform numbers, 60 % of them 1),
masks.associate_det_trk on 243 frames of 8 x 8 masks of 288 x 288, and link_boxes on one and on 32 clips of 243 frames of 8
boxes.  Every device figure is a call through the Python wrapper (output allocation included), HIP events around `reps`
back-to-back calls after two warm-up calls, the median of five such timings (minimum and maximum beside it).

Beside each the reference's way on the same inputs, read-back included: the device tensor's .cpu() and a loop of
scipy.optimize.linear_sum_assignment over the problems (for the association: mask_iou on the device, then per frame the
copy, scipy and the threshold tests on the host; for the tracker: one copy of the boxes, then per frame a NumPy IoU matrix,
scipy and the id bookkeeping).  Those are wall-clock times between two device synchronisations, the median of five after
one warm-up."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from skiing_analysis_pytorch_amd import geometry, masks  # noqa: E402


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


def measure_host(fn, rounds=5):
    fn()
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=float(np.median(t)), ms_min=float(min(t)), ms_max=float(max(t)))


def host_assignment(cost):
    c = cost.cpu().numpy()
    return [linear_sum_assignment(c[b]) for b in range(len(c))]


def host_association(det, trk, scores, thr=0.5):
    out = []
    for t in range(len(det)):
        iou = geometry.mask_iou(det[t], trk[t]).iou
        io, sc = iou.cpu().numpy(), scores[t].cpu().numpy()
        rows, cols = linear_sum_assignment(1 - io)
        matched = {int(k) for r, k in zip(rows, cols) if io[r, k] >= thr}
        new = [d for d in range(len(io)) if not (io[d] >= thr).any() and sc[d] >= 0]
        out.append((new, [k for k in range(io.shape[1]) if k not in matched]))
    return out


def host_tracker(boxes, thr=0.3, max_age=15):
    """the rules of link_boxes on the host, one clip after another: a NumPy IoU matrix and scipy a frame"""
    b_all = boxes.cpu().numpy()
    out = []
    for b in b_all:
        last, age, ids = [], [], np.full(b.shape[:2], -1)
        for t in range(len(b)):
            dets = [d for d in range(b.shape[1]) if np.isfinite(b[t, d]).all()]
            live = [k for k in range(len(last)) if age[k] <= max_age]
            hit = set()
            if dets and live:
                D, L = b[t, dets][:, None, :], np.array([last[k] for k in live])[None, :, :]
                wh = np.clip(np.minimum(D[..., 2:], L[..., 2:]) - np.maximum(D[..., :2], L[..., :2]), 0, None)
                inter = wh[..., 0] * wh[..., 1]
                union = (D[..., 2] - D[..., 0]) * (D[..., 3] - D[..., 1]) + (L[..., 2] - L[..., 0]) * (L[..., 3] - L[..., 1]) - inter
                iou = np.where(union > 0, inter / np.where(union > 0, union, 1), 0)
                for r, k in zip(*linear_sum_assignment(1 - iou)):
                    if iou[r, k] >= thr:
                        ids[t, dets[r]], last[live[k]] = live[k], b[t, dets[r]]
                        hit.add(live[k])
            for d in dets:
                if ids[t, d] < 0:
                    ids[t, d] = len(last)
                    hit.add(len(last))
                    last.append(b[t, d]), age.append(0)
            age = [0 if k in hit else age[k] + 1 for k in range(len(last))]
        out.append(ids)
    return out


def iou_like(B, N, M, g):
    u = torch.rand((B, N, M), device="cuda", generator=g)
    keep = torch.rand((B, N, M), device="cuda", generator=g) >= 0.6
    return (1 - torch.where(keep, u, torch.zeros_like(u))).to(torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []

    def row(name, res, **extra):
        r = dict(call=name, **res, **extra)
        rows.append(r)
        print("  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()), flush=True)

    for B, N, M in ((243, 8, 8), (243, 64, 64), (1, 1024, 1024)):
        c = iou_like(B, N, M, g)
        got = geometry.linear_assignment(c)
        want = np.array([c[b].cpu().numpy()[r, k].sum() for b, (r, k) in enumerate(host_assignment(c))])
        assert int(got.status.sum()) == 0 and np.abs(got.total.cpu().numpy() - want).max() <= 1e-9
        row("linear_assignment", measure(lambda: geometry.linear_assignment(c), a.reps), B=B, N=N, M=M)
        row(".cpu() + scipy loop", measure_host(lambda: host_assignment(c)), B=B, N=N, M=M)

    T, N, h, w = 243, 8, 288, 288
    yy = torch.arange(h, device="cuda")[None, None, :, None]
    xx = torch.arange(w, device="cuda")[None, None, None, :]

    def boxes_as_masks(c, r):
        return ((xx - c[..., 0, None, None]).abs() <= r[..., 0, None, None]) & ((yy - c[..., 1, None, None]).abs() <= r[..., 1, None, None])

    c = torch.randint(60, 228, (T, N, 2), device="cuda", generator=g)
    r = torch.randint(15, 60, (T, N, 2), device="cuda", generator=g)
    det = boxes_as_masks(c, r)
    trk = boxes_as_masks(c + torch.randint(-8, 9, (T, N, 2), device="cuda", generator=g), r)
    scores = torch.rand((T, N), device="cuda", generator=g)
    shape = dict(T=T, N=N, M=N, H=h, W=w)
    row("associate_det_trk", measure(lambda: masks.associate_det_trk(det, trk, det_scores=scores), a.reps), **shape)
    row("mask_iou + per frame .cpu() + scipy", measure_host(lambda: host_association(det, trk, scores)), **shape)

    for B in (1, 32):
        centre = torch.rand((B, 1, N, 2), device="cuda", generator=g, dtype=torch.float64) * 800 + 100
        centre = centre + torch.cumsum(torch.randn((B, T, N, 2), device="cuda", generator=g, dtype=torch.float64) * 4, dim=1)
        size = torch.rand((B, 1, N, 2), device="cuda", generator=g, dtype=torch.float64) * 60 + 30
        boxes = torch.cat([centre - size / 2, centre + size / 2], dim=-1)
        boxes = torch.where(torch.rand((B, T, N, 1), device="cuda", generator=g) < 0.1, torch.full_like(boxes, float("nan")), boxes)
        link = geometry.link_boxes(boxes)
        shape = dict(B=B, T=T, N=N, tracks_mean=float(link.n_tracks.float().mean()))
        row("link_boxes", measure(lambda: geometry.link_boxes(boxes), a.reps), **shape)
        row(".cpu() + NumPy IoU + scipy a frame", measure_host(lambda: host_tracker(boxes)), **shape)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(dict(rows=rows), indent=1))


if __name__ == "__main__":
    main()
