"""The person-centred origin of dense point maps and the camera update that follows it (csrc/person.hip; C-ABI:
skimi_person_origin, skimi_recenter_cameras).

Reference: vggt/multi_view_process.py:195-217 + :356-395.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._args import contig_as, f32, f64, on_device, workspace
from .._lib import SkimiError, check, current_stream, lib, ptr


@dataclass
class PersonOrigin:
    """person_origin's outputs (device tensors, one entry per map; lead = the maps' leading shape)."""
    origin: torch.Tensor    # float64 [..., 3]: mean of the kept points; NaN where nothing was kept
    n_valid: torch.Tensor   # int64 [...]: finite points inside the box
    n_kept: torch.Tensor    # int64 [...]: of those, within 3 sigma of the median depth
    median: torch.Tensor    # float64 [...]
    std: torch.Tensor       # float64 [...]
    stats: torch.Tensor     # float64 [..., 8]: the kernel's record (n_box, n_valid, n_kept, median, std, origin)


def person_stats(points: torch.Tensor, boxes: torch.Tensor, source_size) -> torch.Tensor:
    """the launch of person_origin: points [M, H, W, 3], boxes [M, 4], float32, contiguous, device -> stats [M, 8]"""
    M, H, W, _ = points.shape
    stats = f64(points.device, M, 8)
    ws = workspace(points.device, lib().skimi_person_workspace_bytes(M, H, W), optional=True)
    check(lib().skimi_person_origin(ptr(points), ptr(boxes), M, H, W, int(source_size[0]), int(source_size[1]), ptr(ws),
                                    ptr(stats), current_stream()), "skimi_person_origin")
    return stats


def person_origin(point_maps: torch.Tensor, boxes: torch.Tensor, source_size) -> PersonOrigin:
    """The person-centred origin of dense world-point maps (extract_person_points + the mean its caller takes,
    vggt/multi_view_process.py:356-395, :195-199) without leaving the device: point_maps [..., H, W, 3], boxes [..., 4]
    = (x1, y1, x2, y2) in the pixels of the `source_size` = (height, width) image the detector saw.  Per map: the
    pixels inside the scaled box, finite, within 3 sigma of their median depth (exact median, float64 statistics;
    DESIGN §2 "Person origin") -> their float64 mean."""
    on_device("person_origin", point_maps, boxes)
    if point_maps.dim() < 3 or point_maps.shape[-1] != 3:
        raise SkimiError(f"person_origin: point_maps must be [..., H, W, 3], got {tuple(point_maps.shape)}")
    lead = tuple(point_maps.shape[:-3])
    if tuple(boxes.shape) != lead + (4,):
        raise SkimiError(f"person_origin: boxes must be {list(lead + (4,))}, got {list(boxes.shape)}")
    H, W = point_maps.shape[-3:-1]
    p = contig_as(point_maps.reshape(-1, H, W, 3))
    b = contig_as(boxes.reshape(-1, 4))
    stats = person_stats(p, b, source_size).reshape(*lead, 8)
    return PersonOrigin(stats[..., 5:8], stats[..., 1].to(torch.int64), stats[..., 2].to(torch.int64), stats[..., 3],
                        stats[..., 4], stats)


def recenter_cameras(stats: torch.Tensor, extrinsic: torch.Tensor):
    """The camera update that follows the person origins (multi_view_process.py:201-217), one small launch: stats
    [n, S, 8] (PersonOrigin.stats), extrinsic [n, S, 3, 4] float32 -> (origin [n, 3] float64 = mean of the S origins in
    view order, zero if a view kept nothing; R [n, S, 3, 3], t [n, S, 3] float32 with t_c += R_c origin and, at S = 2,
    view 1 turned by diag(-1, 1, -1) with its t left as the reference's turn-then-mirror leaves it)."""
    on_device("recenter_cameras", stats, extrinsic)
    n, S = extrinsic.shape[:2]
    if tuple(stats.shape) != (n, S, 8) or tuple(extrinsic.shape[2:]) != (3, 4):
        raise ValueError(f"recenter_cameras: need stats [n, S, 8] and extrinsic [n, S, 3, 4], got {list(stats.shape)}, "
                         f"{list(extrinsic.shape)}")
    stats, E = contig_as(stats, torch.float64), contig_as(extrinsic)
    origin, R, t = f64(E.device, n, 3), f32(E.device, n, S, 3, 3), f32(E.device, n, S, 3)
    check(lib().skimi_recenter_cameras(ptr(stats), ptr(E), n, S, ptr(origin), ptr(R), ptr(t), current_stream()),
          "skimi_recenter_cameras")
    return origin, R, t
