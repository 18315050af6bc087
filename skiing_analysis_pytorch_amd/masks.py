"""The reference's mask post-processing under its own names (prepare_front_results/sam3: perflib/connected_components.py,
perflib/masks_ops.py, perflib/nms.py, model/edt.py, model/sam3_tracker_utils.py), on device tensors, and person_boxes, which
turns a clip's person masks into the boxes bev.process_front_clip takes.  Thin mirrors of geometry.mask_components,
distance_transform, mask_inner_point, mask_boxes, mask_iou and nms_greedy (device/masks.py; rules: include/skimi.h, DESIGN §2
"Masks"); the rest is torch ops on the same device.  Only generic_nms synchronises.

associate_det_trk is perflib/associate_det_trk.py for a frame or a clip, on geometry.mask_iou and geometry.linear_assignment
(device/assign.py; DESIGN §2 "Association and tracking") without a read-back; association_lists makes the reference's Python
objects of its result, with one copy.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import geometry


def _binary(t: torch.Tensor) -> torch.Tensor:
    """any tensor -> bool (non-zero = foreground); bool and uint8 pass as they are"""
    return t if t.dtype in (torch.bool, torch.uint8) else t != 0


def connected_components(input: torch.Tensor):
    """perflib/connected_components.py: input [B, H, W] or [B, 1, H, W], non-zero = foreground -> (labels, counts) int32 shaped
    like the input: dense labels (0: background; geometry.mask_components' numbering, 8-connectivity) and the size of each
    pixel's component."""
    if input.dim() not in (3, 4) or (input.dim() == 4 and input.shape[1] != 1):
        raise ValueError(f"connected_components: input must be [B, H, W] or [B, 1, H, W], got {list(input.shape)}")
    m = _binary(input)
    res = geometry.mask_components(m.reshape(m.shape[0], m.shape[-2], m.shape[-1]), 8, 0)
    return res.labels.view(input.shape), res.areas.view(input.shape)


def edt(data: torch.Tensor) -> torch.Tensor:
    """model/edt.py: edt_triton: data [B, H, W], non-zero = foreground -> float32 [B, H, W], the Euclidean distance of every
    pixel to the nearest zero pixel (+inf where the image has none: the project's rule, the reference gives 1e9)."""
    if data.dim() != 3:
        raise ValueError(f"edt: data must be [B, H, W], got {list(data.shape)}")
    return geometry.distance_transform(_binary(data)).dist


def masks_to_boxes(masks: torch.Tensor, obj_ids=None) -> torch.Tensor:
    """perflib/masks_ops.py: masks [N, H, W] -> float32 [N, 4] (x_min, y_min, x_max, y_max) in pixels, inclusive; an empty
    mask gives (W, H, 0, 0)."""
    if masks.dim() != 3 or (obj_ids is not None and len(obj_ids) != masks.shape[0]):
        raise ValueError(f"masks_to_boxes: masks must be [N, H, W] with one obj_id each, got {list(masks.shape)}")
    if masks.numel() == 0:
        return torch.zeros((0, 4), device=masks.device, dtype=torch.float32)
    return geometry.mask_boxes(_binary(masks)).xyxy.to(torch.float32)


def mask_iou(pred_masks: torch.Tensor, gt_masks: torch.Tensor) -> torch.Tensor:
    """perflib/masks_ops.py: pred_masks [N, H, W], gt_masks [M, H, W] bool -> float32 [N, M]"""
    return geometry.mask_iou(pred_masks, gt_masks).iou


def generic_nms(ious: torch.Tensor, scores: torch.Tensor, iou_threshold=0.5) -> torch.Tensor:
    """perflib/nms.py: greedy NMS on a pairwise IoU matrix [N, N] -> the kept indices by decreasing score, int64.  The length
    of the result depends on the data, so THIS FUNCTION SYNCHRONISES (the boolean selection reads the count back);
    geometry.nms_greedy, which it is built on, does not."""
    if ious.dim() != 2 or ious.shape[0] != ious.shape[1] or tuple(scores.shape) != (ious.shape[0],):
        raise ValueError(f"generic_nms: ious [N, N] and scores [N], got {list(ious.shape)}, {list(scores.shape)}")
    keep = geometry.nms_greedy(ious, scores, iou_threshold)
    order = torch.sort(scores.to(torch.float32), descending=True, stable=True).indices
    return order[keep[order]]


def nms_masks(pred_probs: torch.Tensor, pred_masks: torch.Tensor, prob_threshold: float, iou_threshold: float) -> torch.Tensor:
    """perflib/nms.py: pred_probs [num_det], pred_masks [num_det, H, W] scores (foreground: > 0) -> keep bool [num_det]: the
    detections above prob_threshold that survive mask NMS.  The detections below the threshold stay in place as valid=False
    entries: no gather and no read-back."""
    if pred_masks.dim() != 3 or tuple(pred_probs.shape) != (pred_masks.shape[0],):
        raise ValueError(f"nms_masks: pred_probs [num_det] and pred_masks [num_det, H, W], got {list(pred_probs.shape)}, {list(pred_masks.shape)}")
    if pred_probs.numel() == 0:
        return pred_probs > prob_threshold
    binary = pred_masks > 0
    return geometry.nms_greedy(geometry.mask_iou(binary, binary).iou, pred_probs, iou_threshold, valid=pred_probs > prob_threshold)


def small_components(binary: torch.Tensor, area_thresh) -> torch.Tensor:
    """binary [B, 1, H, W] bool -> bool: the foreground pixels whose 8-connected component has at most area_thresh pixels
    (a number, or a tensor broadcastable to [B, 1, H, W])"""
    areas = geometry.mask_components(binary[:, 0], 8, 0).areas[:, None]
    return binary & (areas <= area_thresh)


def fill_holes_in_mask_scores(mask: torch.Tensor, max_area: int, fill_holes: bool = True, remove_sprinkles: bool = True) -> torch.Tensor:
    """model/sam3_tracker_utils.py: mask scores [B, 1, H, W] float.  Background components (mask <= 0) of at most max_area
    pixels become 0.1; then foreground components (> 0) of at most min(foreground area // 2, max_area) pixels become -0.1.
    max_area <= 0 returns the input."""
    if max_area <= 0:
        return mask
    if mask.dim() != 4 or mask.shape[1] != 1:
        raise ValueError(f"fill_holes_in_mask_scores: mask must be [B, 1, H, W], got {list(mask.shape)}")
    if fill_holes:
        mask = torch.where(small_components(mask <= 0, max_area), 0.1, mask)
    if remove_sprinkles:
        fg = mask > 0
        thresh = torch.sum(fg, dim=(2, 3), keepdim=True, dtype=torch.int32).floor_divide_(2).clamp_(max=max_area)
        mask = torch.where(small_components(fg, thresh), -0.1, mask)
    return mask


def sample_one_point_from_error_center(gt_masks: torch.Tensor, pred_masks, padding: bool = True):
    """model/sam3_tracker_utils.py: gt_masks, pred_masks [B, 1, H, W] bool (pred_masks None: no prediction) -> (points int64
    [B, 1, 2] (x, y), labels int64 [B, 1]): the innermost pixel of the false negative region (label 1) or of the false positive
    region (label 0), whichever lies deeper; positive iff the false negatives' squared distance is STRICTLY larger (compared
    exactly, as integers).  padding: the outside of the image counts as zero."""
    if pred_masks is None:
        pred_masks = torch.zeros_like(gt_masks)
    if gt_masks.dtype != torch.bool or gt_masks.dim() != 4 or gt_masks.shape[1] != 1 or pred_masks.dtype != torch.bool or pred_masks.shape != gt_masks.shape:
        raise ValueError(f"sample_one_point_from_error_center: gt_masks and pred_masks must be bool [B, 1, H, W], got {list(gt_masks.shape)}")
    fp = (~gt_masks & pred_masks)[:, 0]
    fn = (gt_masks & ~pred_masks)[:, 0]
    fn_xy, fn_d2 = geometry.mask_inner_point(fn, border_zero=padding)
    fp_xy, fp_d2 = geometry.mask_inner_point(fp, border_zero=padding)
    positive = fn_d2 > fp_d2
    points = torch.where(positive[:, None], fn_xy, fp_xy).to(torch.int64)
    return points[:, None], positive.to(torch.int64)[:, None]


Association = namedtuple("Association", "trk_to_det trk_matched trk_unmatched det_new det_trk trk_det_scores")


def associate_det_trk(det_masks, track_masks, iou_threshold=0.5, iou_threshold_trk=0.5, det_scores=None, new_det_thresh=0.0,
                      n_det=None, n_trk=None, iou=None, trk_nonempty=None) -> Association:
    """perflib/associate_det_trk.py (and the matching of model/sam3_video_base.py: _associate_det_trk) for a frame or a whole
    clip, without a read-back: det_masks [N, H, W], track_masks [M, H, W] (foreground: > 0; bool passes as it is), or both with
    a clip axis [T, ...]; det_scores [.., N] is required (with None the reference fails at det_scores_list[d]).  n_det, n_trk
    int32 [T] (a frame: 0-d): the frame has that many detections and tracks, the rest of its rows and columns is padding.
    iou float32 [.., N, M]: an already computed geometry.mask_iou(...).iou; the masks may then be None.  Both mask sets must
    have the same size: the reference's bilinear resize of unequal sizes is not reproduced.

    The cost is the reference's 1 - iou in float32, widened, and geometry.linear_assignment solves it; where the optimum is not
    unique the assignment may differ from scipy's (DESIGN §2 "Association and tracking").  -> Association of device tensors:
    trk_to_det int32 [.., M] (-1: none); trk_matched bool: assigned and iou >= iou_threshold_trk; trk_unmatched bool: not
    matched, and with trk_nonempty bool [.., M] given sam3_video_base's rule, non-empty and not matched; det_new bool [.., N]:
    no track with iou >= iou_threshold and score >= new_det_thresh (a frame without tracks: every detection, as the
    reference's early return); det_trk bool [.., N, M] = iou >= iou_threshold, the reference's det_to_matched_trk as a mask;
    trk_det_scores float32 [.., M, 2]: score and score * iou of the assigned detection, NaN where none is assigned."""
    fn = "associate_det_trk"
    if det_scores is None:
        raise ValueError(f"{fn}: det_scores is required")
    if iou is None:
        if det_masks.shape[-2:] != track_masks.shape[-2:]:
            raise ValueError(f"{fn}: det_masks and track_masks must have one size, got {list(det_masks.shape)}, {list(track_masks.shape)}")
        det, trk = (m if m.dtype in (torch.bool, torch.uint8) else m > 0 for m in (det_masks, track_masks))
        if det.shape[-3] == 0 or trk.shape[-3] == 0:    # no pair at all
            iou = torch.zeros((*det.shape[:-2], trk.shape[-3]), dtype=torch.float32, device=det.device)
        else:
            iou = geometry.mask_iou(det, trk).iou
    if not isinstance(iou, torch.Tensor) or iou.dtype != torch.float32 or iou.dim() not in (2, 3):
        raise ValueError(f"{fn}: iou must be float32 [N, M] or [T, N, M]")
    if tuple(det_scores.shape) != tuple(iou.shape[:-1]):
        raise ValueError(f"{fn}: det_scores must be {list(iou.shape[:-1])}, got {list(det_scores.shape)}")
    dev, lead = iou.device, tuple(iou.shape[:-2])
    N, M = int(iou.shape[-2]), int(iou.shape[-1])
    nd = torch.full(lead, N, dtype=torch.int32, device=dev) if n_det is None else n_det.to(dev, torch.int32).reshape(lead)
    nt = torch.full(lead, M, dtype=torch.int32, device=dev) if n_trk is None else n_trk.to(dev, torch.int32).reshape(lead)
    det_ok = torch.arange(N, device=dev) < nd[..., None]
    trk_ok = torch.arange(M, device=dev) < nt[..., None]
    scores = det_scores.to(dev, torch.float32)

    trk_to_det = geometry.linear_assignment(1 - iou, nd, nt).col_to_row
    at = trk_to_det.clamp(min=0).to(torch.int64)[..., None, :]
    assigned = trk_to_det >= 0
    if N:
        pair_iou = torch.gather(iou, -2, at)[..., 0, :]
        pair_score = torch.gather(scores[..., :, None].expand(*lead, N, M), -2, at)[..., 0, :]
    else:
        pair_iou = pair_score = torch.zeros((*lead, M), dtype=torch.float32, device=dev)
    trk_matched = assigned & (pair_iou >= iou_threshold_trk)
    trk_unmatched = trk_ok & ~trk_matched
    if trk_nonempty is not None:
        trk_unmatched = trk_unmatched & trk_nonempty.to(dev, torch.bool)
    det_trk = (iou >= iou_threshold) & det_ok[..., :, None] & trk_ok[..., None, :]
    det_new = det_ok & ((~det_trk.any(dim=-1) & (scores >= new_det_thresh)) | (nt == 0)[..., None])
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    trk_det_scores = torch.where(assigned[..., None], torch.stack([pair_score, pair_score * pair_iou], dim=-1), nan)
    return Association(trk_to_det, trk_matched, trk_unmatched, det_new, det_trk, trk_det_scores)


def association_lists(result: Association):
    """One frame's Association -> the reference's four Python objects (new_det_indices, unmatched_trk_indices,
    det_to_matched_trk, matched_det_scores), read back in one copy.  A frame without detections or without tracks gives the
    reference's early return: every detection new and nothing else."""
    if result.trk_to_det.dim() != 1:
        raise ValueError("association_lists: one frame at a time (index the clip axis of every field first)")
    N, M = int(result.det_new.shape[0]), int(result.trk_to_det.shape[0])
    if N == 0 or M == 0:
        return list(range(N)), [], {}, {}
    flat = torch.cat([result.trk_to_det.to(torch.float64), result.trk_unmatched.to(torch.float64), result.det_new.to(torch.float64),
                      result.det_trk.reshape(-1).to(torch.float64), result.trk_det_scores.reshape(-1).to(torch.float64)]).cpu().numpy()
    t2d, unm, new, dt, sc = flat[:M], flat[M:2 * M], flat[2 * M:2 * M + N], flat[2 * M + N:2 * M + N + N * M], flat[2 * M + N + N * M:]
    dt, sc = dt.reshape(N, M), sc.reshape(M, 2)
    det_to_matched_trk = {d: [t for t in range(M) if dt[d, t]] for d in range(N) if dt[d].any()}
    # in the order the reference fills its dictionary: by detection
    matched_det_scores = {t: [float(sc[t, 0]), float(sc[t, 1])] for t in sorted((t for t in range(M) if t2d[t] >= 0), key=lambda t: t2d[t])}
    return [d for d in range(N) if new[d]], [t for t in range(M) if unm[t]], det_to_matched_trk, matched_det_scores


def largest_component_boxes(stats: torch.Tensor, W: int, H: int):
    """mask_components' stats [..., C, 7] -> (boxes_xywh float64 [..., 4], area int32 [...]): the component of largest area, ties
    to the lowest label, as SAM3 writes out_boxes_xywh: (x_min, y_min, x_max - x_min, y_max - y_min) / (W, H, W, H); no
    component: a NaN box and area 0.  Plain torch ops on whatever device stats is on."""
    C = int(stats.shape[-2])
    if C == 0:
        raise ValueError("largest_component_boxes: the stats table has no rows")
    area = stats[..., 0]
    # one integer key: the area first, then the lower row
    best = torch.argmax(area * C + (C - 1 - torch.arange(C, device=stats.device)), dim=-1)
    row = torch.gather(stats, -2, best[..., None, None].expand(*best.shape, 1, 7))[..., 0, :]
    box = torch.stack([row[..., 1], row[..., 2], row[..., 3] - row[..., 1], row[..., 4] - row[..., 2]], dim=-1).to(torch.float64)
    box = box / torch.tensor([W, H, W, H], dtype=torch.float64, device=stats.device)
    box = torch.where((row[..., 0] > 0)[..., None], box, torch.full_like(box, float("nan")))
    return box, row[..., 0].to(torch.int32)


def person_boxes(masks: torch.Tensor, max_area: int = 0, max_components: int = 256):
    """masks [T, N, H, W] bool or uint8 on the device -> (boxes_xywh float64 [T, N, 4], area int32 [T, N]): every mask is
    optionally cleaned (max_area > 0: fill_holes_in_mask_scores' two passes), its largest 8-connected component is taken
    (among the first max_components in raster order; ties to the lowest label) and that component's box is returned as SAM3
    writes out_boxes_xywh, which is what bev.process_front_clip takes.  A mask without foreground gives a NaN box.  Nothing
    is read back."""
    if masks.dim() != 4:
        raise ValueError(f"person_boxes: masks must be [T, N, H, W], got {list(masks.shape)}")
    T, N, H, W = (int(s) for s in masks.shape)
    m = _binary(masks).reshape(T * N, H, W)
    if max_area > 0:
        scores = torch.where(m != 0, 1.0, -1.0)[:, None]
        m = fill_holes_in_mask_scores(scores, max_area)[:, 0] > 0
    stats = geometry.mask_components(m, 8, max_components).stats
    box, area = largest_component_boxes(stats, W, H)
    return box.view(T, N, 4), area.view(T, N)
