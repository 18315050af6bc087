"""Association and tracking (csrc/assign.hip, csrc/lsap.h; C-ABI: skimi_linear_assignment, skimi_link_boxes): a batch of
rectangular linear assignment problems in one launch, and persistent ids for the boxes of a batch of clips; masks.
associate_det_trk and tracks.py are built on these; rules: include/skimi.h, DESIGN §2 "Association and tracking".

Nothing is read back, the launches of a call depend on the shapes only, and every problem's (clip's) result is bitwise what
it is alone.  A batch of no problems gives empty results without a launch.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from .._args import f64, i32, strip_lead
from .._lib import check, current_stream, lib, ptr

ASSIGN_MAX = 1024
LINK_MAX = 64

Assignment = namedtuple("Assignment", "row_to_col col_to_row total status")
LinkedBoxes = namedtuple("LinkedBoxes", "ids n_tracks table overflow")


def _device(fn, **named):
    for name, t in named.items():
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"{fn}: {name} must be a device tensor (it is on {getattr(t, 'device', 'the host')})")


def _counts(fn, name, n, B, limit, dev):
    """None, or the int32 [B] counts of a ragged batch on the device"""
    if n is None:
        return None
    if n.dtype != torch.int32 or tuple(n.shape) != (B,):
        raise ValueError(f"{fn}: {name} must be int32 [{B}] (at most {limit} each), got {n.dtype} {list(n.shape)}")
    return n.to(dev).contiguous()


def linear_assignment(cost: torch.Tensor, n_rows=None, n_cols=None, maximize: bool = False) -> Assignment:
    """A batch of rectangular assignment problems: cost float32 or float64 [B, N, M] on the device (float32 is widened, which is
    exact), n_rows, n_cols int32 [B] on the device or None: problem b is the top-left n_rows[b] x n_cols[b] block, either may
    be 0 -> row_to_col int32 [B, N], col_to_row int32 [B, M] (-1: unassigned; exactly min(n_rows, n_cols) pairs), total
    float64 [B] = the assigned costs summed in ascending row order, status int32 [B] = 1 iff the block holds a NaN or an
    infinity (the maps are then -1 and total NaN).  One [N, M] matrix (with 0-d counts) gives results without the leading axis.

    The pairs minimise the total; maximize=True solves -cost (total is then the sum of the negated costs).  Shortest augmenting
    paths with float64 duals, the method of scipy.optimize.linear_sum_assignment; among equal distances the LOWEST column is
    taken, so where the optimum is not unique the pairs may differ from scipy's (the totals agree).  N, M <= ASSIGN_MAX.  One
    launch, a wave a problem."""
    fn = "linear_assignment"
    if not isinstance(cost, torch.Tensor) or cost.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{fn}: cost must be a float32 or float64 tensor, got {getattr(cost, 'dtype', type(cost))}")
    if cost.dim() not in (2, 3):
        raise ValueError(f"{fn}: cost must be [N, M] or [B, N, M], got {list(cost.shape)}")
    single = cost.dim() == 2
    c = cost[None] if single else cost
    B, N, M = (int(s) for s in c.shape)
    if N > ASSIGN_MAX or M > ASSIGN_MAX:
        raise ValueError(f"{fn}: N = {N}, M = {M}, at most {ASSIGN_MAX} each")
    if B >= 2 ** 31:
        raise ValueError(f"{fn}: B = {B} problems, at most 2^31 - 1")
    _device(fn, cost=cost, n_rows=n_rows, n_cols=n_cols)
    dev = c.device
    if single:
        n_rows, n_cols = (None if n is None else n.reshape(-1) for n in (n_rows, n_cols))
    nr, nc = _counts(fn, "n_rows", n_rows, B, N, dev), _counts(fn, "n_cols", n_cols, B, M, dev)
    c = c.to(torch.float64)
    c = (-c if maximize else c).contiguous()
    res = Assignment(i32(dev, B, N), i32(dev, B, M), f64(dev, B), i32(dev, B))
    if B and N and M:
        check(lib().skimi_linear_assignment(ptr(c), ptr(nr), ptr(nc), B, N, M, ptr(res.row_to_col), ptr(res.col_to_row), ptr(res.total),
                                            ptr(res.status), current_stream()), "skimi_linear_assignment")
    else:   # no rows or no columns: nothing to assign
        res.row_to_col.fill_(-1), res.col_to_row.fill_(-1), res.total.zero_(), res.status.zero_()
    return Assignment(*strip_lead(res, single))


def link_boxes(boxes: torch.Tensor, scores=None, iou_threshold: float = 0.3, max_age: int = 15, new_score: float = 0.0,
               max_tracks: int = LINK_MAX) -> LinkedBoxes:
    """Persistent ids over a clip: boxes float64 [B, T, N, 4] on the device, (x1, y1, x2, y2) in pixels, a box with a non-finite
    coordinate is "no detection"; scores [B, T, N] or None -> ids int32 [B, T, N] (-1: none), n_tracks int32 [B], table int32
    [B, K, 3] = first frame, last frame, hits of every track (-1, -1, 0 behind n_tracks), overflow int32 [B]; K = max_tracks.
    One [T, N, 4] clip gives results without the leading axis.  Frame by frame (include/skimi.h has the arithmetic):
     1. the live tracks are those seen at most max_age frames ago, in ascending id order;
     2. cost[d, k] = 1 - IoU(box d, the last box of track k) in float64, solved by linear_assignment's rules;
     3. an assigned pair with IoU >= iou_threshold gives the detection the track's id and the track the detection's box; every
        other valid detection with score >= new_score starts a track with the next id, in detection-index order;
     4. ids are never reused; when K tracks exist further detections get -1 and overflow counts them;
     5. a track not matched ages by one.
    N, K <= LINK_MAX.  One launch, a wave a clip; no motion model."""
    fn = "link_boxes"
    if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float64:
        raise ValueError(f"{fn}: boxes must be a float64 tensor, got {getattr(boxes, 'dtype', type(boxes))}")
    if boxes.dim() not in (3, 4) or boxes.shape[-1] != 4:
        raise ValueError(f"{fn}: boxes must be [T, N, 4] or [B, T, N, 4], got {list(boxes.shape)}")
    single = boxes.dim() == 3
    bx = (boxes[None] if single else boxes).contiguous()
    B, T, N = (int(s) for s in bx.shape[:3])
    K = int(max_tracks)
    if not 1 <= K <= LINK_MAX or N > LINK_MAX:
        raise ValueError(f"{fn}: N = {N} boxes a frame and max_tracks = {max_tracks!r}: at most {LINK_MAX} each, at least one track")
    if int(max_age) < 0 or iou_threshold != iou_threshold or new_score != new_score:
        raise ValueError(f"{fn}: max_age = {max_age!r} (>= 0), iou_threshold = {iou_threshold!r}, new_score = {new_score!r}")
    if B * T * N >= 2 ** 31:
        raise ValueError(f"{fn}: {B * T * N} boxes, at most 2^31 - 1")
    _device(fn, boxes=boxes, scores=scores)
    sc = None
    if scores is not None:
        if not scores.dtype.is_floating_point or tuple(scores.shape) != tuple(boxes.shape[:-1]):
            raise ValueError(f"{fn}: scores must be floating point {list(boxes.shape[:-1])}, got {scores.dtype} {list(scores.shape)}")
        sc = scores.to(bx.device, torch.float64).contiguous()
    dev = bx.device
    res = LinkedBoxes(i32(dev, B, T, N), i32(dev, B), i32(dev, B, K, 3), i32(dev, B))
    if B and T and N:
        check(lib().skimi_link_boxes(ptr(bx), ptr(sc), B, T, N, K, float(iou_threshold), int(max_age), float(new_score), ptr(res.ids),
                                     ptr(res.n_tracks), ptr(res.table), ptr(res.overflow), current_stream()), "skimi_link_boxes")
    else:   # no frames or no boxes: no tracks
        res.ids.fill_(-1), res.n_tracks.zero_(), res.overflow.zero_()
        res.table.copy_(torch.tensor([-1, -1, 0], dtype=torch.int32, device=dev))
    return LinkedBoxes(*strip_lead(res, single))
