"""A person's boxes over a clip, on the device: geometry.link_boxes gives every detection a persistent id (csrc/assign.hip;
rules: include/skimi.h, DESIGN §2 "Association and tracking"), and the helpers here, plain torch ops without a read-back,
turn the ids into the per-person layout bev.process_front_clip takes.  select_person_boxes is the device counterpart of the
reference's YOLOv11Bbox.__call__ (prepare_dataset/model/yolov11_bbox.py).
"""
from __future__ import annotations

import torch

from .geometry import LINK_MAX, LinkedBoxes, link_boxes  # noqa: F401  (re-exports)


def track_boxes(ids: torch.Tensor, boxes: torch.Tensor, K: int) -> torch.Tensor:
    """ids int32 [.., T, N] (link_boxes), boxes [.., T, N, 4] in any convention -> [.., T, K, 4]: the box of track k in slot k of
    every frame, NaN where the track is absent (integer boxes are made float64).  With masks.person_boxes' normalised xywh
    this is the [T, N, 4] layout bev.process_front_clip takes: slot k is one person in every frame."""
    if tuple(ids.shape) != tuple(boxes.shape[:-1]) or boxes.shape[-1] != 4 or ids.dim() < 2:
        raise ValueError(f"track_boxes: ids [.., T, N] and boxes [.., T, N, 4], got {list(ids.shape)}, {list(boxes.shape)}")
    K = int(K)
    if K < 1:
        raise ValueError(f"track_boxes: K = {K}, at least one slot")
    b = boxes if boxes.dtype.is_floating_point else boxes.to(torch.float64)
    # a track appears at most once a frame: slot K takes what has no id and is cut off
    out = torch.full((*ids.shape[:-1], K + 1, 4), float("nan"), dtype=b.dtype, device=b.device)
    slot = torch.where((ids >= 0) & (ids < K), ids, K).to(torch.int64)
    out.scatter_(-2, slot[..., None].expand(*slot.shape, 4), b)
    return out[..., :K, :]


def main_track(table: torch.Tensor) -> torch.Tensor:
    """link_boxes' table int32 [.., K, 3] -> int64 [..]: the track with the most hits, ties to the lowest id (0 when there is no
    track: its slot is then empty in every frame)"""
    K = int(table.shape[-2])
    hits = table[..., 2].to(torch.int64)
    return torch.argmax(hits * K + (K - 1 - torch.arange(K, device=table.device)), dim=-1)


def select_person_boxes(boxes: torch.Tensor, scores=None, iou_threshold: float = 0.3, max_age: int = 15, new_score: float = 0.0,
                        max_tracks: int = LINK_MAX):
    """boxes float64 [T, N, 4] xyxy in pixels (a non-finite box: no detection), scores [T, N] or None -> (bbox float64 [T, 4],
    missing bool [T]): the clip's main track (the one seen in the most frames, ties to the lowest id), its box in every frame;
    the frames where it is absent are NaN and flagged.  With a batch axis [B, T, N, 4] -> [B, T, 4], [B, T].

    This REPLACES the reference's rule rather than reproducing it: YOLOv11Bbox picks, frame by frame, the box whose centre is
    nearest to the previous frame's (its own comment calls this a fallback without an id-keeping mechanism, and the choice
    jumps to the other skier when two cross), and fills the missing frames from their neighbours (process_none).  Neither is
    done here: the ids come from link_boxes' assignment on IoU, and a missing frame stays missing."""
    link = link_boxes(boxes, scores, iou_threshold, max_age, new_score, max_tracks)
    per_track = track_boxes(link.ids, boxes, int(max_tracks))
    k = main_track(link.table)
    bbox = torch.gather(per_track, -2, k[..., None, None, None].expand(*per_track.shape[:-2], 1, 4))[..., 0, :]
    return bbox, torch.isnan(bbox).any(dim=-1)
