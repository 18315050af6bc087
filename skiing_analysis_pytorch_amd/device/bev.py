"""The bird's-eye view on points: homography fit and transfer, the skeleton on the plan, the ground track (csrc/bev.hip;
C-ABI: skimi_homography_fit, skimi_homography_points, skimi_bev_skeleton, skimi_ground_track; the frames'
skimi_warp_perspective_u8 is bound in preprocess.py): front_side/front/bev_utils.py, front_side/run.py:153-197, :222-255;
the reference's names and the clip entry point are the package's bev.py; rules: include/skimi.h, DESIGN §2 "Bird's-eye
view".
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from .._args import add_lead, f64, f64_dev, host_f64, host_ptr, i32, on_device, strip_lead, u8
from .._lib import check, current_stream, lib, ptr

HOMOGRAPHY_STAT_FIELDS = ("n_used", "rms_err", "max_err", "det")
TRACK_FIELDS = ("step", "path", "vx", "vy", "speed", "heading")


@dataclass
class HomographyResult:
    """homography_fit's outputs (device tensors; a leading group axis only when the input had one)."""
    H: torch.Tensor          # float64 [.., 3, 3]: post @ Hn, maps src to post's frame; NaN for a failed group
    Hinv: torch.Tensor       # float64 [.., 3, 3]: adj(H) / det(H), what preprocess.warp_perspective takes
    Hn: torch.Tensor         # float64 [.., 3, 3]: the fit itself, before post (the reference's H_m beside H_px = S @ H_m)
    err: torch.Tensor        # float64 [.., n]: transfer error of every used point in post's frame, NaN for an unused one
    stats: torch.Tensor      # float64 [.., 4]: HOMOGRAPHY_STAT_FIELDS (det is that of Hn, before post)
    status: torch.Tensor     # bool [..]: Hn finite and |det Hn| >= 1e-12 (the reference's check_homography)


class BevSkeletonResult(NamedTuple):
    """bev_skeleton's outputs (device tensors)."""
    uv: torch.Tensor             # float64 [T, J, 2]: unrounded plan pixels, NaN for an invalid joint
    px: torch.Tensor             # int32 [T, J, 2]: rounded half to even, 0 for an invalid joint
    valid: torch.Tensor          # bool [T, J]
    center_world: torch.Tensor   # float64 [T, 3]: np.nanmean over the joints per coordinate


class GroundTrackResult(NamedTuple):
    """ground_track's outputs (device tensors, views of `table`)."""
    table: torch.Tensor      # float64 [P, T, 6]: TRACK_FIELDS
    step: torch.Tensor       # [P, T] metres moved since the previous sample (0 at t = 0, NaN next to a gap)
    path: torch.Tensor       # [P, T] the running sum of the finite steps
    velocity: torch.Tensor   # [P, T, 2] metres per second, central differences
    speed: torch.Tensor      # [P, T]
    heading: torch.Tensor    # [P, T] atan2(vx, vy): 0 along +y (down the lane), positive towards +x


def homography_fit(src: torch.Tensor, dst: torch.Tensor, post=None) -> HomographyResult:
    """cv2.findHomography(src, dst, method=0) without its Levenberg-Marquardt polish, for G independent groups in one launch:
    src, dst [n, 2] or [G, n, 2] device tensors, n >= 4 (a correspondence with a non-finite number is skipped); post a host
    [3, 3] composed on the left (H = post @ Hn: the canvas matrix S of bev.make_bev_canvas) -> HomographyResult.  Hartley
    normalisation, the 9 x 9 normal matrix, cyclic Jacobi, the eigenvector of the smallest eigenvalue: for n > 4 the
    algebraic least-squares solution; RANSAC and LMedS are out.  A degenerate group (fewer than 4 usable points, all points
    of a side coincident, |det| < 1e-12) is NaN with status False; the others are not affected.  Nothing is read back."""
    s, d = f64_dev("homography_fit", src), f64_dev("homography_fit", dst)
    if s.dim() not in (2, 3) or s.shape[-1] != 2 or d.shape != s.shape:
        raise ValueError(f"homography_fit: src and dst must both be [n, 2] or [G, n, 2], got {list(s.shape)}, {list(d.shape)}")
    (s, single), d = add_lead(s, 3), add_lead(d, 3)[0]
    G, n = int(s.shape[0]), int(s.shape[1])
    if n < 4 or G < 1:
        raise ValueError(f"homography_fit: at least 4 correspondences and one group, got n = {n}, G = {G}")
    ph = None
    if post is not None:
        ph = host_f64(post)
        if ph.shape != (3, 3) or not np.isfinite(ph).all():
            raise ValueError(f"homography_fit: post must be a finite [3, 3], got shape {list(ph.shape)}")
    dev = s.device
    H, Hinv, Hn, err, stats, status = f64(dev, G, 3, 3), f64(dev, G, 3, 3), f64(dev, G, 3, 3), f64(dev, G, n), f64(dev, G, 4), i32(dev, G)
    check(lib().skimi_homography_fit(ptr(s), ptr(d), host_ptr(ph), G, n, ptr(H), ptr(Hinv), ptr(Hn), ptr(err), ptr(stats), ptr(status),
                                     current_stream()), "skimi_homography_fit")
    return HomographyResult(*strip_lead((H, Hinv, Hn, err, stats, status.bool()), single))


def homography_points(x: torch.Tensor, H: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """bev_utils.image_points_to_bev in one launch: x [..., n, 2] and H device tensors -> float64 [..., n, 2].  H [3, 3] serves
    every point; H [..., 3, 3] with x's leading axes gives every group of n points its own (a matrix per frame).  Where the
    reference raises (|w| < eps) and where the point or w is not finite, the point is NaN in both coordinates and no other."""
    on_device("homography_points", H, what="the matrices on the device")
    xi = f64_dev("homography_points", x)
    Hd = f64_dev("homography_points", H, x.device)
    if xi.dim() < 1 or xi.shape[-1] != 2:
        raise ValueError(f"homography_points: points must be [..., 2], got {list(xi.shape)}")
    if tuple(Hd.shape) == (3, 3):
        shared, G, n = 1, 1, xi.numel() // 2
    else:
        if xi.dim() < 2 or Hd.shape[-2:] != (3, 3) or tuple(Hd.shape[:-2]) != tuple(xi.shape[:-2]):
            raise ValueError(f"homography_points: H must be [3, 3] or match the points' leading axes, got H {list(Hd.shape)} "
                             f"for points {list(xi.shape)}")
        shared, n = 0, int(xi.shape[-2])
        G = xi.numel() // 2 // n if n else 0
    if not float(eps) >= 0.0:
        raise ValueError(f"homography_points: eps must be >= 0, got {eps}")
    out = torch.empty_like(xi)
    check(lib().skimi_homography_points(ptr(xi), ptr(Hd), G, n, shared, float(eps), ptr(out), current_stream()),
          "skimi_homography_points")
    return out


def bev_skeleton(X: torch.Tensor, center_px: torch.Tensor, metres_per_pixel: float = 0.02, use_axes=(0, 2),
                 rot90_left: bool = False, center_world=None) -> BevSkeletonResult:
    """front_side/run.py: project_world_to_bev_centered with merge's centre, for a whole clip in one launch: X [T, J, 3] (or
    [J, 3]) world joints, center_px [T, 2] (or [2]) the plan pixel the skeleton is centred on (merge: the last box's foot
    point), device tensors -> BevSkeletonResult.  The centre in the world is np.nanmean over the joints per coordinate; a
    joint with a non-finite coordinate (the reference's None), or a step whose centre is not finite, is invalid: NaN in
    uv, 0 in px.  px rounds half to even, as Python's round does in the reference.  center_world [T, 3] (device): a centre of
    the caller's in place of the mean."""
    Xd, single = add_lead(f64_dev("bev_skeleton", X), 3)
    if Xd.dim() != 3 or Xd.shape[2] != 3 or Xd.shape[1] < 1:
        raise ValueError(f"bev_skeleton: need X [T, J, 3], got {list(X.shape)}")
    T, J, dev = int(Xd.shape[0]), int(Xd.shape[1]), Xd.device
    c = f64_dev("bev_skeleton", center_px, dev)
    if tuple(c.shape) not in ((T, 2), (2,) if single else (T, 2)):
        raise ValueError(f"bev_skeleton: center_px must be [{T}, 2], got {list(c.shape)}")
    ax0, ax1 = (int(a) for a in use_axes)
    if not (0 <= ax0 <= 2 and 0 <= ax1 <= 2):
        raise ValueError(f"bev_skeleton: use_axes must be two of 0, 1, 2, got {use_axes}")
    if not float(metres_per_pixel) > 0.0:
        raise ValueError(f"bev_skeleton: metres_per_pixel must be positive, got {metres_per_pixel}")
    cin = None
    if center_world is not None:
        cin = f64_dev("bev_skeleton", center_world, dev)
        if tuple(cin.shape) not in ((T, 3), (3,) if single else (T, 3)):
            raise ValueError(f"bev_skeleton: center_world must be [{T}, 3], got {list(cin.shape)}")
    uv, px, valid, cw = f64(dev, T, J, 2), i32(dev, T, J, 2), u8(dev, T, J), f64(dev, T, 3)
    check(lib().skimi_bev_skeleton(ptr(Xd), ptr(c), ptr(cin), T, J, float(metres_per_pixel), ax0, ax1, int(bool(rot90_left)), ptr(uv), ptr(px),
                                   ptr(valid), ptr(cw), current_stream()), "skimi_bev_skeleton")
    return BevSkeletonResult(*strip_lead((uv, px, valid.bool(), cw), single))


def ground_track(p: torch.Tensor, fps: float = 30.0) -> GroundTrackResult:
    """The metric ground track of P people in one launch: p [P, T, 2] (or [T, 2]) positions on the ground plane in metres
    (bev.process_front_clip's foot_m), NaN = no detection -> GroundTrackResult: the step and the path length, the velocity
    by central differences (one-sided at the two ends), the speed and the heading atan2(vx, vy).  A value next to a gap is
    NaN; the path sums the finite steps only.  NOTHING IS SMOOTHED INSIDE: a box's foot point jitters by pixels, which the
    differences amplify, so smooth the track first with smooth_savgol or smooth_ema (as [T, P, 3] with a zero third
    coordinate) and pass the result."""
    pd, single = add_lead(f64_dev("ground_track", p), 3)
    if pd.dim() != 3 or pd.shape[2] != 2:
        raise ValueError(f"ground_track: need p [P, T, 2], got {list(p.shape)}")
    if not float(fps) > 0.0:
        raise ValueError(f"ground_track: fps must be positive, got {fps}")
    P, T = int(pd.shape[0]), int(pd.shape[1])
    out = f64(pd.device, P, T, 6)
    check(lib().skimi_ground_track(ptr(pd), P, T, float(fps), ptr(out), current_stream()), "skimi_ground_track")
    out, = strip_lead((out,), single)
    return GroundTrackResult(out, out[..., 0], out[..., 1], out[..., 2:4], out[..., 4], out[..., 5])
