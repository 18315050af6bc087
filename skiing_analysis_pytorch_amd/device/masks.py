"""Mask analysis (csrc/masks.hip; C-ABI: skimi_mask_*, skimi_nms_greedy): connected components, the exact Euclidean distance
transform and its inner point, boxes, pairwise IoU and greedy NMS on device masks; the reference's names (the package's
masks.py) are built on these; rules: include/skimi.h, DESIGN §2 "Masks".

A mask is a bool or uint8 device tensor [B, H, W], non-zero = foreground; one [H, W] mask gives results without the leading
axis.  Nothing is read back, the launches of a call depend on the shapes only, and every mask's result is bitwise what it is
for that mask alone.  A batch of no masks gives empty results without a launch.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from .._args import f32, i32, i64, mask_batch, strip_lead, u8
from .._lib import check, current_stream, lib, ptr

MASK_MAX_SIDE = 4096
EDT_NONE = 1 << 30
NMS_MAX = 1024
STATS_FIELDS = ("area", "x_min", "y_min", "x_max", "y_max", "sum_x", "sum_y")

ComponentsResult = namedtuple("ComponentsResult", "labels areas count stats")
EdtResult = namedtuple("EdtResult", "d2 dist")
MaskBoxes = namedtuple("MaskBoxes", "xyxy area")
MaskIoU = namedtuple("MaskIoU", "iou inter union")


def mask_components(masks: torch.Tensor, connectivity: int = 8, max_components: int = 256) -> ComponentsResult:
    """Connected components of masks [B, H, W] -> labels int32 [B, H, W] (0: background; 1 .. count[b] in the raster order of
    the components' first pixels, scipy.ndimage.label's numbering), areas int32 [B, H, W] (the pixel count of the pixel's
    component), count int32 [B], stats int64 [B, max_components, 7] (STATS_FIELDS of components 1 .. max_components, zero
    behind count; max_components=0: no table, stats is [B, 0, 7]).  connectivity: 4 or 8."""
    m, single = mask_batch("mask_components", masks)
    if connectivity not in (4, 8):
        raise ValueError(f"mask_components: connectivity must be 4 or 8, got {connectivity!r}")
    maxc = int(max_components)
    B, H, W = (int(s) for s in m.shape)
    if maxc < 0 or B * maxc >= 2 ** 31:
        raise ValueError(f"mask_components: max_components = {max_components!r}")
    dev = m.device
    res = ComponentsResult(i32(dev, B, H, W), i32(dev, B, H, W), i32(dev, B), i64(dev, B, maxc, 7))
    if B:
        nbytes = lib().skimi_mask_components_workspace_bytes(B, H, W)
        ws = u8(dev, nbytes)
        check(lib().skimi_mask_components(ptr(m), B, H, W, int(connectivity), maxc, ptr(res.labels), ptr(res.areas), ptr(res.count),
                                          ptr(res.stats) if maxc else None, ptr(ws), nbytes, current_stream()), "skimi_mask_components")
    return ComponentsResult(*strip_lead(res, single))


def distance_transform(masks: torch.Tensor, border_zero: bool = False) -> EdtResult:
    """The exact Euclidean distance transform of masks [B, H, W] -> d2 int32 [B, H, W], the squared distance from each pixel to
    the nearest zero pixel of its mask (0 on zero pixels), and dist float32 = sqrt(d2).  border_zero: every position outside
    the image counts as zero.  A mask without any zero (border_zero=False) gives d2 = EDT_NONE and dist = +inf."""
    m, single = mask_batch("distance_transform", masks)
    B, H, W = (int(s) for s in m.shape)
    res = EdtResult(i32(m.device, B, H, W), f32(m.device, B, H, W))
    if B:
        check(lib().skimi_mask_edt(ptr(m), B, H, W, int(bool(border_zero)), ptr(res.d2), ptr(res.dist), current_stream()), "skimi_mask_edt")
    return EdtResult(*strip_lead(res, single))


def mask_inner_point(masks: torch.Tensor, border_zero: bool = True):
    """The pixel farthest from the mask's zeros -> (xy int32 [B, 2], d2 int32 [B]): the largest d2 of distance_transform, ties
    to the first in raster order (the argmax over the flattened transform); a mask of zeros gives (0, 0) and 0."""
    m, single = mask_batch("mask_inner_point", masks)
    B, H, W = (int(s) for s in m.shape)
    dev = m.device
    xy, best = i32(dev, B, 2), i32(dev, B)
    if B:
        d2 = i32(dev, B, H, W)
        check(lib().skimi_mask_edt(ptr(m), B, H, W, int(bool(border_zero)), ptr(d2), None, current_stream()), "skimi_mask_edt")
        check(lib().skimi_mask_argmax(ptr(d2), B, H, W, ptr(xy), ptr(best), current_stream()), "skimi_mask_argmax")
    return strip_lead((xy, best), single)


def pack_masks(m: torch.Tensor) -> torch.Tensor:
    """mask_batch's uint8 masks [..., H, W] -> int64 [..., ceil(H W / 64)]: bit i of word k = pixel 64 k + i of the flattened
    mask, the last word zero-filled (the layout mask_boxes and mask_iou read)"""
    lead, HW = tuple(m.shape[:-2]), int(m.shape[-2]) * int(m.shape[-1])
    words = i64(m.device, *lead, (HW + 63) // 64)
    B = m.numel() // HW
    if B:
        check(lib().skimi_mask_pack(ptr(m), B, HW, ptr(words), current_stream()), "skimi_mask_pack")
    return words


def mask_boxes(masks: torch.Tensor) -> MaskBoxes:
    """masks [N, H, W] -> xyxy int32 [N, 4], the inclusive pixel extremes (x_min, y_min, x_max, y_max), and area int32 [N]; an
    empty mask gives (W, H, 0, 0) and 0, the arithmetic of the reference's masks_to_boxes."""
    m, single = mask_batch("mask_boxes", masks)
    B, H, W = (int(s) for s in m.shape)
    res = MaskBoxes(i32(m.device, B, 4), i32(m.device, B))
    if B:
        words = pack_masks(m)
        check(lib().skimi_mask_boxes(ptr(words), B, H, W, ptr(res.xyxy), ptr(res.area), current_stream()), "skimi_mask_boxes")
    return MaskBoxes(*strip_lead(res, single))


def mask_iou(a: torch.Tensor, b: torch.Tensor) -> MaskIoU:
    """Pairwise IoU of a [N, H, W] and b [M, H, W] -> iou float32, inter, union int32 [N, M]; with a leading clip axis
    [T, N, H, W], [T, M, H, W] -> [T, N, M].  iou = float32(inter) / float32(max(union, 1)), the reference's formula.  Every
    mask is packed once into 64-bit words; a pair is popcounts of AND and OR."""
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dim() != b.dim():
        raise ValueError(f"mask_iou: a and b must have the same number of axes, got {list(a.shape)}, {list(b.shape)}")
    ma, single = mask_batch("mask_iou", a, 4, "a")
    mb, _ = mask_batch("mask_iou", b, 4, "b")
    if ma.shape[0] != mb.shape[0] or ma.shape[2:] != mb.shape[2:] or ma.device != mb.device:
        raise ValueError(f"mask_iou: a [T, N, H, W] and b [T, M, H, W] on one device, got {list(a.shape)}, {list(b.shape)}")
    T, N, M = int(ma.shape[0]), int(ma.shape[1]), int(mb.shape[1])
    if T > 65535 or T * N * M >= 2 ** 31:
        raise ValueError(f"mask_iou: T = {T}, N = {N}, M = {M}: at most 65535 clips and 2^31 - 1 pairs")
    dev = ma.device
    res = MaskIoU(f32(dev, T, N, M), i32(dev, T, N, M), i32(dev, T, N, M))
    if T * N * M:
        wa, wb = pack_masks(ma), pack_masks(mb)
        check(lib().skimi_mask_iou(ptr(wa), ptr(wb), T, N, M, int(wa.shape[-1]), ptr(res.iou), ptr(res.inter), ptr(res.union),
                                   current_stream()), "skimi_mask_iou")
    return MaskIoU(*strip_lead(res, single))


def nms_greedy(iou: torch.Tensor, scores: torch.Tensor, iou_threshold: float, valid=None) -> torch.Tensor:
    """Greedy NMS on an IoU matrix: iou float32 [N, N], scores [N], valid bool [N] or None -> keep bool [N]; with a clip axis
    [T, N, N], [T, N] -> [T, N].  Entries are visited by score descending, ties to the lower index; a kept i suppresses every
    later j with iou[i, j] > iou_threshold (compared in float32).  Entries with valid == False or a NaN score are not kept and
    suppress nothing.  N <= NMS_MAX.  One launch, nothing read back."""
    for name, t in (("iou", iou), ("scores", scores), ("valid", valid)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise ValueError(f"nms_greedy: {name} must be a device tensor (it is on {getattr(t, 'device', 'the host')})")
    if not iou.dtype.is_floating_point or not scores.dtype.is_floating_point:
        raise ValueError(f"nms_greedy: iou and scores must be floating point, got {iou.dtype}, {scores.dtype}")
    single = iou.dim() == 2
    if iou.dim() not in (2, 3) or iou.shape[-1] != iou.shape[-2] or tuple(scores.shape) != tuple(iou.shape[:-1]):
        raise ValueError(f"nms_greedy: iou [N, N] with scores [N], or [T, N, N] with [T, N], got {list(iou.shape)}, {list(scores.shape)}")
    if valid is not None and (tuple(valid.shape) != tuple(scores.shape) or valid.dtype not in (torch.bool, torch.uint8)):
        raise ValueError(f"nms_greedy: valid must be bool {list(scores.shape)}, got {valid.dtype} {list(valid.shape)}")
    N = int(iou.shape[-1])
    if N > NMS_MAX:
        raise ValueError(f"nms_greedy: N = {N}, at most {NMS_MAX}")
    dev = iou.device
    if scores.numel() == 0:
        return torch.zeros(tuple(scores.shape), dtype=torch.bool, device=dev)
    io = iou.to(torch.float32).contiguous().reshape(-1, N, N)
    sc = scores.to(dev, torch.float32).contiguous().reshape(-1, N)
    va = None if valid is None else valid.to(dev).contiguous().view(torch.uint8).reshape(-1, N)
    T = int(io.shape[0])
    keep = u8(dev, T, N)
    if T * N:
        check(lib().skimi_nms_greedy(ptr(io), ptr(sc), ptr(va), T, N, float(iou_threshold), ptr(keep), current_stream()), "skimi_nms_greedy")
    keep = keep.view(torch.bool)
    return keep[0] if single else keep
