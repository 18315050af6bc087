"""The front camera's bird's-eye view (BEV): the front half of the reference's front/side pipeline
(front_side/run.py: process_one_person) on the device.

Four marked ground points give a homography onto a metric ground plane; every frame is warped into the plan, every box's
foot point is mapped to plan pixels and to metres, the side views' skeleton is placed on the plan, and the metric ground
track (path length, speed, heading: merge's open TODO) is taken from the foot points.  The names and signatures follow
front_side/front/bev_utils.py (copied as prepare_front_results/bev_utils.py), front_side/front/run.py and
front_side/run.py, minus files: nothing here writes PNGs (as angle.py), and process_front_clip draws nothing; draw_points
marks points on a clip with the device rasteriser (geometry.draw_shapes, DESIGN §2 "Drawing").

The kernels are csrc/bev.hip (rules: include/skimi.h, DESIGN §2 "Bird's-eye view"), reached through geometry.homography_fit,
geometry.homography_points, preprocess.warp_perspective, geometry.bev_skeleton and geometry.ground_track.  Box
arithmetic (xywh -> xyxy, the foot point) is plain torch on the device; every matrix of process_front_clip, H_px, H_m and the
warp's inverse, comes out of the one fit launch.  Frames and boxes must be device tensors.

process_front_clip differs from the reference in ONE deliberate way: the reference resizes every frame to the
calibration size (1920 x 1080) and then warps it, two resamplings; here the pixel-centre scaling of that resize is
folded into the matrix (the ground points are carried into the frame's own pixels and fitted there) and the frame is
sampled once (see its docstring).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import geometry, preprocess
from ._args import device_tensor

# the reference's marked ground points of the 1920 x 1080 front frame and their places on the ground, in metres
DEFAULT_IMG_PTS = np.array([[0.0, 1080.0], [1920.0, 1080.0], [1336.0, 130.0], [600.0, 130.0]], dtype=np.float64)
DEFAULT_BEV_PTS_M = np.array([[-15.0, 0.0], [15.0, 0.0], [15.0, 60.0], [-15.0, 60.0]], dtype=np.float64)
MERGE_METRES_PER_PIXEL = 0.02     # front_side/run.py: merge


@dataclass
class BeVConfig:
    lane_width_m: float = 30.0
    lane_length_m: float = 60.0
    px_per_m: float = 20.0
    margin_x_m: float = 5.0
    margin_y_m: float = 10.0


def make_bev_canvas(cfg: BeVConfig = BeVConfig()) -> Tuple[Tuple[int, int], np.ndarray]:
    """-> ((width, height) of the plan in pixels, S [3, 3] float64: metres -> plan pixels, y pointing up the plan)."""
    x_min = -cfg.lane_width_m / 2 - cfg.margin_x_m
    x_max = +cfg.lane_width_m / 2 + cfg.margin_x_m
    y_min = 0.0 - cfg.margin_y_m
    y_max = cfg.lane_length_m + cfg.margin_y_m
    w = int(np.ceil((x_max - x_min) * cfg.px_per_m))
    h = int(np.ceil((y_max - y_min) * cfg.px_per_m))
    s = cfg.px_per_m
    return (w, h), np.array([[s, 0, -x_min * s], [0, -s, y_max * s], [0, 0, 1]], dtype=np.float64)


def convert_xywh_to_xyxy(bboxes_xywh: torch.Tensor) -> torch.Tensor:
    """[..., 4] (x, y, w, h) -> (x1, y1, x2, y2) = (x, y, x + w, y + h)."""
    b = device_tensor("convert_xywh_to_xyxy", bboxes_xywh)
    if b.dim() < 1 or b.shape[-1] != 4:
        raise ValueError(f"Invalid bbox shape for xywh to xyxy: {list(b.shape)}")
    return torch.stack([b[..., 0], b[..., 1], b[..., 0] + b[..., 2], b[..., 1] + b[..., 3]], dim=-1)


def unnormalize_bbox(bbox: torch.Tensor, img_size: Tuple[int, int]) -> torch.Tensor:
    """[..., 4] (x1, y1, x2, y2) in [0, 1] -> float64 pixels of img_size = (H, W)."""
    b = device_tensor("unnormalize_bbox", bbox).to(torch.float64)
    if b.dim() < 1 or b.shape[-1] != 4:
        raise ValueError(f"bbox last dim must be 4, got {list(b.shape)}")
    H, W = img_size
    return b * torch.tensor([W, H, W, H], dtype=torch.float64, device=b.device)


def foot_from_bbox_xyxy(bbox: torch.Tensor) -> torch.Tensor:
    """[..., 4] (x1, y1, x2, y2) -> float64 [..., 2]: the middle of the box's lower edge, ((x1 + x2) * 0.5, y2)."""
    b = device_tensor("foot_from_bbox_xyxy", bbox).to(torch.float64)
    if b.dim() < 1 or b.shape[-1] != 4:
        raise ValueError(f"bbox must have 4 numbers, got {list(b.shape)}")
    return torch.stack([(b[..., 0] + b[..., 2]) * 0.5, b[..., 3]], dim=-1)


def image_points_to_bev(uv: torch.Tensor, H: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """uv [..., n, 2] through H [3, 3] (or one H per leading index): geometry.homography_points.  Where the reference raises
    (a homogeneous coordinate below eps) the point is NaN."""
    return geometry.homography_points(uv, H, eps)


def inverse3(H: torch.Tensor) -> torch.Tensor:
    """adj(H) / det(H) of a [3, 3] device matrix, cofactor by cofactor as skimi_homography_fit's rule 8: for
    warp_image_to_bev alone, which is handed cv2's forward matrix; a fit's own inverse is HomographyResult.Hinv."""
    h = H.reshape(9)
    a, b, c, d, e, f, g, hh, i = (h[k] for k in range(9))
    det = a * (e * i - f * hh) - b * (d * i - f * g) + c * (d * hh - e * g)
    adj = torch.stack([e * i - f * hh, c * hh - b * i, b * f - c * e,
                       f * g - d * i, a * i - c * g, c * d - a * f,
                       d * hh - e * g, b * g - a * hh, a * e - b * d])
    return (adj / det).reshape(3, 3)


def warp_image_to_bev(image: torch.Tensor, H: torch.Tensor, bev_size: Tuple[int, int]) -> torch.Tensor:
    """cv2.warpPerspective(image, H, bev_size, flags=INTER_LINEAR): image uint8 [h, w, ch] or [F, h, w, ch], H [3, 3] the
    FORWARD matrix (image -> plan) as cv2 takes it, both on the device; bev_size = (width, height)."""
    img = device_tensor("warp_image_to_bev", image)
    Hd = device_tensor("warp_image_to_bev", H).to(torch.float64)
    if tuple(Hd.shape) != (3, 3):
        raise ValueError(f"H shape must be (3,3), got {list(Hd.shape)}")
    out = preprocess.warp_perspective(img if img.dim() == 4 else img[None], inverse3(Hd), bev_size)
    return out if img.dim() == 4 else out[0]


def point_shapes(pts: torch.Tensor, color=(0, 0, 255), radius=4, labels=None) -> torch.Tensor:
    """draw_points' shape list: pts [..., N, 2] -> int32 [..., N + characters, 8]: the N filled discs, then the labels (str(i + 1)
    unless `labels` names them), in the points' colour at scale 2, from (+8, -8) of the point.  The reference converts the
    points with np.asarray(dtype=int32), which truncates towards zero: so does this.  A non-finite point is left out."""
    p = torch.as_tensor(pts).to(torch.float64)
    if p.dim() < 2 or p.shape[-1] != 2:
        raise ValueError(f"pts must be [..., N, 2], got {list(p.shape)}")
    N = int(p.shape[-2])
    names = [str(i + 1) for i in range(N)] if labels is None else [str(s) for s in labels]
    if len(names) != N:
        raise ValueError(f"draw_points: {len(names)} labels for {N} points")
    q = torch.trunc(p)      # NaN stays NaN: kind 0 in both builders
    off = torch.tensor([8.0, -8.0], dtype=torch.float64, device=p.device)
    return geometry.cat_shapes(geometry.disc_shapes(q, radius, color), geometry.text_shapes(names, q + off, 2, color))


def draw_points(frames: torch.Tensor, pts: torch.Tensor, color=(0, 0, 255), radius=4, labels=None) -> torch.Tensor:
    """front_side/front/bev_utils.py: draw_points for a whole clip in one launch: frames uint8 [F, H, W, ch], pts [N, 2] (the
    same points on every frame) or [F, N, 2], device tensors -> the drawn frames (a new tensor): a filled disc per point and
    its number (labels: other strings).  Drawn by geometry.draw_shapes under the project's own anti-aliasing and font (DESIGN
    §2 "Drawing"), not cv2's.  Nothing is read back."""
    fr = device_tensor("draw_points", frames)
    return geometry.draw_shapes(fr, point_shapes(device_tensor("draw_points", pts).to(fr.device), color, radius, labels))


def check_homography(H) -> None:
    """The reference's check, raising ValueError; a device tensor is read back (this synchronises: inside a clip use
    HomographyResult.status, which skimi_homography_fit sets by the same rule, instead)."""
    if H is None or tuple(H.shape) != (3, 3):
        raise ValueError("H is invalid")
    Hh = H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else np.asarray(H)
    Hh = Hh.astype(np.float64)
    if not np.isfinite(Hh).all():
        raise ValueError("H contains NaN/Inf")
    det = (Hh[0, 0] * (Hh[1, 1] * Hh[2, 2] - Hh[1, 2] * Hh[2, 1]) - Hh[0, 1] * (Hh[1, 0] * Hh[2, 2] - Hh[1, 2] * Hh[2, 0])
           + Hh[0, 2] * (Hh[1, 0] * Hh[2, 1] - Hh[1, 1] * Hh[2, 0]))
    if abs(det) < 1e-12:
        raise ValueError("H is near-singular")


def _img_pts(img_pts) -> np.ndarray:
    if img_pts is None:
        return DEFAULT_IMG_PTS
    p = np.asarray(img_pts.detach().cpu().numpy() if isinstance(img_pts, torch.Tensor) else img_pts, dtype=np.float32)
    if p.shape != (4, 2):
        raise ValueError(f"img_pts must be (4,2), got {p.shape}")
    return p.astype(np.float64)     # through float32 as the reference


def _blank(n, h, w, bg, device) -> torch.Tensor:
    return torch.tensor(bg, dtype=torch.uint8, device=device).expand(n, h, w, 3).contiguous()


def make_bev(img: torch.Tensor, bboxes_xyxy: torch.Tensor, img_pts=None, cfg: BeVConfig = BeVConfig(), blank_bev: bool = False,
             bev_bg=(10, 10, 10)):
    """One frame: img uint8 [h, w, 3] in the calibration's own size and bboxes_xyxy [N, 4] (or [4]) pixels, on the device ->
    (foot_xy_px float64 [N, 2] plan pixels, src = img as it came, bev_img uint8 [bev_h, bev_w, 3]).  blank_bev: the plan is
    the flat colour bev_bg and nothing is warped.  A degenerate img_pts raises ValueError as the reference (one read-back
    of the fit's status; process_front_clip reads nothing back)."""
    img = device_tensor("make_bev", img)
    boxes = device_tensor("make_bev", bboxes_xyxy).to(torch.float64)
    if boxes.dim() == 1:
        boxes = boxes[None]
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError(f"bboxes_xyxy must be (N,4), got {list(boxes.shape)}")
    dev = img.device
    bev_size, S = make_bev_canvas(cfg)
    fit = geometry.homography_fit(torch.from_numpy(_img_pts(img_pts)).to(dev), torch.from_numpy(DEFAULT_BEV_PTS_M).to(dev), post=S)
    if not bool(fit.status):
        raise ValueError("H is near-singular or contains NaN/Inf")
    if blank_bev:
        bev_img = _blank(1, bev_size[1], bev_size[0], bev_bg, dev)[0]
    else:
        bev_img = preprocess.warp_perspective(img[None], fit.Hinv, bev_size)[0]
    return image_points_to_bev(foot_from_bbox_xyxy(boxes), fit.H), img, bev_img


def project_world_to_bev_centered(kpts_world: torch.Tensor, center_world, center_px, meters_per_pixel: float, use_axes=(0, 2),
                                  rot90_left: bool = False) -> geometry.BevSkeletonResult:
    """kpts_world [J, 3] (or [T, J, 3]), center_world [3] ([T, 3]; None: merge's np.nanmean over the joints), center_px [2]
    ([T, 2]), device tensors -> BevSkeletonResult.  The reference's list of (u, v) tuples and None is px with valid."""
    k = device_tensor("project_world_to_bev_centered", kpts_world)
    c = center_px if isinstance(center_px, torch.Tensor) else torch.tensor([float(v) for v in center_px], dtype=torch.float64,
                                                                          device=k.device)
    return geometry.bev_skeleton(k, c, meters_per_pixel, use_axes, rot90_left, center_world=center_world)


@dataclass
class FrontClipResult:
    """process_front_clip's outputs (device tensors)."""
    bev: torch.Tensor              # uint8 [T, bev_h, bev_w, 3]: every frame in the plan (blank_bev: the flat colour)
    foot_uv: torch.Tensor          # float64 [T, N, 2]: the boxes' foot points, pixels of the calibration frame
    foot_px: torch.Tensor          # float64 [T, N, 2]: in plan pixels (the reference's foot_xy_px)
    foot_m: torch.Tensor           # float64 [T, N, 2]: on the ground, metres
    track: geometry.GroundTrackResult   # of every box index: [N, T, ..] from foot_m (smoothed first when smooth is set)
    H_px: torch.Tensor             # float64 [3, 3]: calibration-frame pixels -> plan pixels, S @ H_m (the fit's H)
    H_m: torch.Tensor              # float64 [3, 3]: calibration-frame pixels -> metres (the fit's Hn)
    status: torch.Tensor           # bool []: the reference's check_homography on H_m
    skeleton: Optional[geometry.BevSkeletonResult]   # the side views' skeleton on the plan, when skeleton was given
    bev_size: Tuple[int, int]      # (width, height)


def process_front_clip(frames: torch.Tensor, boxes_xywh: torch.Tensor, img_pts=None, cfg: BeVConfig = BeVConfig(),
                       calib_size=(1080, 1920), fps: float = 30, blank_bev: bool = False, skeleton: Optional[torch.Tensor] = None,
                       smooth: Optional[str] = None, bev_bg=(10, 10, 10)) -> FrontClipResult:
    """front/run.py: process_front_frame + bev_utils.make_bev + the centre of front_side/run.py: merge for a whole clip:
    frames uint8 [T, h, w, 3], boxes_xywh [T, N, 4] normalised (x, y, w, h) as SAM3 gives them, device tensors; img_pts the
    four marked ground points in pixels of the calibration frame calib_size = (H, W) -> FrontClipResult.  One fit launch
    (two groups), one points launch, one warp launch and one track launch for the clip; nothing is read back.

    skeleton [T, J, 3]: world joints of the side views, placed on the plan around the LAST box's foot point with merge's
    0.02 m/px and rot90_left.  smooth: None, "savgol" or "ema": the foot track in metres is smoothed (geometry.
    smooth_savgol / smooth_ema) before the differences of geometry.ground_track, which smooths nothing itself.

    THE ONE DELIBERATE DIFFERENCE from the reference: it resizes every frame to calib_size (cv2.resize, bilinear) and then
    warps the result, two resamplings.  Here a frame of another size is sampled once: cv2.resize maps a pixel centre of its
    output to src = (dst + 0.5) s - 0.5 with s = size / calib size; that scaling A is folded into the matrix, H_actual =
    H_px A^-1: the second group of the fit takes the ground points A img_pts, in the frame's own pixels, and its Hinv is
    what the warp reads the frame with.  For frames already of calib_size A is the identity, the two groups are the same
    bits and the result is the reference's rule exactly."""
    fr = device_tensor("process_front_clip", frames)
    if fr.dtype != torch.uint8 or fr.dim() != 4 or fr.shape[3] != 3:
        raise ValueError(f"process_front_clip: frames must be uint8 [T, h, w, 3], got {fr.dtype} {list(fr.shape)}")
    boxes = device_tensor("process_front_clip", boxes_xywh)
    T, h, w = int(fr.shape[0]), int(fr.shape[1]), int(fr.shape[2])
    if boxes.dim() != 3 or boxes.shape[0] != T or boxes.shape[2] != 4:
        raise ValueError(f"process_front_clip: boxes_xywh must be [{T}, N, 4], got {list(boxes.shape)}")
    if smooth not in (None, "savgol", "ema"):
        raise ValueError(f"process_front_clip: smooth must be None, 'savgol' or 'ema', got {smooth!r}")
    dev = fr.device
    Hc, Wc = int(calib_size[0]), int(calib_size[1])
    bev_size, S = make_bev_canvas(cfg)

    foot_uv = foot_from_bbox_xyxy(unnormalize_bbox(convert_xywh_to_xyxy(boxes.to(torch.float64)), (Hc, Wc)))
    pts = _img_pts(img_pts)
    sx, sy = w / Wc, h / Hc
    own = pts if (h, w) == (Hc, Wc) else (pts + 0.5) * np.array([sx, sy]) - 0.5     # the ground points in the frame's own pixels
    fit = geometry.homography_fit(torch.from_numpy(np.stack([pts, own])).to(dev),
                                  torch.from_numpy(np.stack([DEFAULT_BEV_PTS_M, DEFAULT_BEV_PTS_M])).to(dev), post=S)
    H_px, H_m = fit.H[0], fit.Hn[0]
    both = image_points_to_bev(foot_uv.reshape(1, -1, 2).expand(2, -1, 2).contiguous(), torch.stack([H_px, H_m]))
    foot_px, foot_m = both[0].reshape(foot_uv.shape), both[1].reshape(foot_uv.shape)

    if blank_bev:
        bev = _blank(T, bev_size[1], bev_size[0], bev_bg, dev)
    else:
        bev = preprocess.warp_perspective(fr, fit.Hinv[1], bev_size)

    p = foot_m
    if smooth is not None and T:
        X3 = torch.cat([foot_m, torch.zeros_like(foot_m[..., :1])], dim=-1)
        p = (geometry.smooth_savgol(X3).X if smooth == "savgol" else geometry.smooth_ema(X3).X)[..., :2]
    track = geometry.ground_track(p.permute(1, 0, 2).contiguous(), fps)

    skel = None
    if skeleton is not None:
        if boxes.shape[1] < 1:
            raise ValueError("process_front_clip: a skeleton needs at least one box to centre it on")
        skel = geometry.bev_skeleton(skeleton, foot_px[:, -1].contiguous(), MERGE_METRES_PER_PIXEL, (0, 2), True)
    return FrontClipResult(bev, foot_uv, foot_px, foot_m, track, H_px, H_m, fit.status[0], skel, bev_size)


# ---- the top-down skeleton video (front_side/o3d_bev_video_robust.py) --------------------------------------------------------
COCO_EDGES = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 7), (7, 9), (6, 8), (8, 10), (5, 6), (5, 11), (6, 12), (11, 12), (11, 13), (13, 15),
              (12, 14), (14, 16)]


@dataclass
class BevView:
    """The reference's BevView (the offscreen backend's fields): the camera sits eye_height above lookat on the world's +y and
    looks down at it; `up` is the screen's up direction."""
    up: Tuple[float, float, float] = (0.0, 0.0, -1.0)
    lookat: Tuple[float, float, float] = (0.0, 0.0, 10.0)
    eye_height: float = 25.0
    fov_deg: float = 60.0                # Open3D's default vertical field of view


def render_bev_skeleton_clip(kpts_world: torch.Tensor, edges=COCO_EDGES, view: BevView = BevView(), size=(720, 1280), line_width=3.0,
                             grid=((15.0, 30.0), 5.0)) -> torch.Tensor:
    """Open3DBevVideoRenderer without the video file: kpts_world [T, J, 3] device joints -> the frames uint8 [T, H, W, 3] (RGB):
    the skeleton's edges in the reference's green, line_width pixels wide, on white, seen top-down from eye_height above
    view.lookat (perspective, the reference's 1280 x 720 by default); the ground, a lit box in the reference, is a grey grid
    on the plane y = 0 ((half extents in x and z around lookat, spacing); None: no grid).  One render_scene call for the
    clip; nothing is read back."""
    k = device_tensor("render_bev_skeleton_clip", torch.as_tensor(kpts_world))
    if k.dim() != 3 or k.shape[-1] != 3:
        raise ValueError(f"render_bev_skeleton_clip: kpts_world must be [T, J, 3], got {list(k.shape)}")
    H, W = int(size[0]), int(size[1])
    dev, T = k.device, int(k.shape[0])
    look = torch.tensor(view.lookat, dtype=torch.float64, device=dev)
    eye = look + torch.tensor([0.0, view.eye_height, 0.0], dtype=torch.float64, device=dev)
    f = (H / 2.0) / float(np.tan(np.radians(view.fov_deg) / 2.0))
    v = geometry.look_at_view(eye, look, torch.tensor(view.up, dtype=torch.float64, device=dev), f, f, W / 2.0, H / 2.0,
                              0.01 * view.eye_height, 4.0 * view.eye_height)
    J = int(k.shape[1])
    ok = [(int(a), int(b)) for a, b in edges if 0 <= int(a) < J and 0 <= int(b) < J]
    ia = torch.tensor([e[0] for e in ok], dtype=torch.int64, device=dev)
    ib = torch.tensor([e[1] for e in ok], dtype=torch.int64, device=dev)
    lists = []
    if grid is not None:
        lists.append(geometry.grid_prims("xz", grid[0], grid[1], v, (235, 235, 235), 1.0, level=0.0, origin=(view.lookat[0], view.lookat[2])))
    lists.append(geometry.segment3d_prims(k.index_select(1, ia), k.index_select(1, ib), v, (0, 255, 0), line_width))
    return geometry.render_scene(v[None].expand(T, -1).contiguous(), prims=geometry.cat_prims(*lists), size=(H, W),
                                 background=(255, 255, 255)).frames
