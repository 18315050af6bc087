"""The filtered, coloured scene cloud of a time step (csrc/scene.hip; C-ABI: skimi_scene_tile, skimi_scene_workspace_bytes,
skimi_scene_cloud): predictions_to_glb restated, vggt/visual_util.py:39-236; rules: DESIGN §2 "Scene cloud".
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .._args import contig_as, f32, f64, on_device, shapes, u8, workspace
from .._lib import check, current_stream, lib, ptr

SCENE_MAX_PIXELS = (2 ** 31 - 1) // 3


class SceneCloud(NamedTuple):
    """scene_point_cloud's outputs (device tensors, B scenes of n pixels, cap rows each)."""
    xyz: torch.Tensor          # float32 [B, cap, 3]: the kept vertices in pixel order (aligned or raw); rows >= count unwritten
    rgb: torch.Tensor          # uint8 [B, cap, 3]
    count: torch.Tensor        # int64 [B]: the full number kept (may exceed cap)
    threshold: torch.Tensor    # float64 [B]
    lower: torch.Tensor        # float64 [B, 3]: 5th percentile of the raw kept vertices per axis
    upper: torch.Tensor        # float64 [B, 3]: 95th
    scale: torch.Tensor        # float64 [B]: ||upper - lower||; 1 for an empty scene
    transform: torch.Tensor    # float64 [B, 4, 4]: E0^-1 diag(-1, -1, 1, 1)
    n_nan_conf: torch.Tensor   # int64 [B]
    n_nonfinite: torch.Tensor  # int64 [B]: kept vertices with a non-finite coordinate
    stats: torch.Tensor        # float64 [B, 16]: the kernel's record (thr, lo, hi, ...; include/skimi.h)


def scene_launch(n: int):
    """The launch geometry of scene_point_cloud for a scene of n pixels: (workgroups per scene, consecutive pixels each
    handles per pass)."""
    n = int(n)
    tile = int(lib().skimi_scene_tile(n))
    if tile <= 0:
        raise ValueError(f"scene_launch: a scene holds 1..{SCENE_MAX_PIXELS} pixels, got {n}")
    return (n + tile - 1) // tile, tile


def scene_point_cloud(points: torch.Tensor, conf: torch.Tensor, images: torch.Tensor, extrinsic: torch.Tensor,
                      conf_thres: float = 50.0, mask_black_bg: bool = False, mask_white_bg: bool = False, align: bool = True,
                      capacity=None, out=None) -> SceneCloud:
    """The point cloud predictions_to_glb builds (vggt/visual_util.py:39-236) for B time steps in one call, without
    leaving the device: points [B, S, H, W, 3], conf [B, S, H, W], images [B, S, 3, H, W] or [B, S, H, W, 3] (the
    reference's test: shape[2] == 3 means channels first), extrinsic [B, S, 3, 4].  Per scene: uint8 colours, the
    conf_thres-th percentile of the confidences as threshold (exact, float64), the kept pixels compacted in pixel order,
    the 5th / 95th percentile box of the kept vertices and its diagonal (the scene scale), and the alignment E0^-1
    diag(-1, -1, 1, 1), applied to the written vertices when align.  capacity (default S H W) bounds the rows written per
    scene; `count` is the full number kept.  out=(xyz, rgb): write into these tensors ([B, capacity, 3] float32 / uint8)
    instead of allocating them.  Rules: DESIGN §2 "Scene cloud"."""
    on_device("scene_point_cloud", points=points, conf=conf, images=images, extrinsic=extrinsic)
    if points.dim() != 5 or points.shape[-1] != 3:
        raise ValueError(f"scene_point_cloud: points must be [B, S, H, W, 3], got {list(points.shape)}")
    B, S, H, W, _ = points.shape
    if B < 1 or S < 1 or H < 1 or W < 1:
        raise ValueError(f"scene_point_cloud: need B >= 1, S >= 1 and a non-empty map, got points {list(points.shape)}")
    n = S * H * W
    if n > SCENE_MAX_PIXELS:
        raise ValueError(f"scene_point_cloud: a scene holds at most {SCENE_MAX_PIXELS} pixels, got {n}")
    shapes("scene_point_cloud", (("conf", conf, (B, S, H, W)),))
    if images.dim() != 5:
        raise ValueError(f"scene_point_cloud: images must be [B, S, 3, H, W] or [B, S, H, W, 3], got {list(images.shape)}")
    nchw = images.shape[2] == 3   # the reference's `images.shape[1] == 3` on one scene
    if tuple(images.shape) != ((B, S, 3, H, W) if nchw else (B, S, H, W, 3)):
        raise ValueError(f"scene_point_cloud: images must be [B, S, 3, H, W] or [B, S, H, W, 3] for points "
                         f"{list(points.shape)}, got {list(images.shape)}")
    shapes("scene_point_cloud", (("extrinsic", extrinsic, (B, S, 3, 4)),))
    q = float(conf_thres)
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"scene_point_cloud: conf_thres is a percentile in [0, 100], got {conf_thres}")
    cap = n if capacity is None else int(capacity)
    if cap < 1:
        raise ValueError(f"scene_point_cloud: capacity must be at least 1, got {capacity}")
    dev = points.device
    points, conf, images, extrinsic = (contig_as(a) for a in (points, conf, images, extrinsic))
    if out is None:
        xyz, rgb = f32(dev, B, cap, 3), u8(dev, B, cap, 3)
    else:
        xyz, rgb = out
        for a, dt in ((xyz, torch.float32), (rgb, torch.uint8)):
            if not a.is_cuda or a.dtype != dt or tuple(a.shape) != (B, cap, 3) or not a.is_contiguous():
                raise ValueError(f"scene_point_cloud: out must be contiguous device tensors {[B, cap, 3]} float32 / uint8")
    count = torch.empty((B,), dtype=torch.int64, device=dev)
    stats, transform = f64(dev, B, 16), f64(dev, B, 4, 4)
    ws = workspace(dev, lib().skimi_scene_workspace_bytes(B, n))
    check(lib().skimi_scene_cloud(ptr(points), ptr(conf), ptr(images), ptr(extrinsic), B, S, H, W, 1 if nchw else 0, q,
                                  1 if mask_black_bg else 0, 1 if mask_white_bg else 0, 1 if align else 0, cap, ptr(ws), ptr(xyz),
                                  ptr(rgb), ptr(count), ptr(stats), ptr(transform), current_stream()), "skimi_scene_cloud")
    return SceneCloud(xyz, rgb, count, stats[:, 0], stats[:, 5:8], stats[:, 8:11], stats[:, 11], transform,
                      stats[:, 3].to(torch.int64), stats[:, 4].to(torch.int64), stats)
