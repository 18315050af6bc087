"""The reference's drawing functions on whole device clips: keypoints with their skeleton, and the reprojection panel.

Every stage of the reference ends by drawing its result on the frames with cv2.circle / cv2.line / cv2.putText, frame by
frame and joint by joint on the host.  Here the frames, the keypoints and the reprojections are device tensors already, and
a clip is drawn in one launch of the rasteriser (geometry.draw_shapes, csrc/draw.hip): these functions only build the
ordered shape lists, with torch ops on the device, in the order the reference draws.  They take no file arguments and
write no images.  bev.draw_points is the third of the family.

The anti-aliasing and the 5 x 7 font are the project's own rules (DESIGN §2 "Drawing"): the pictures show what the
reference's show, in the same places, colours and order; they are not pixel copies of cv2's LINE_AA and Hershey output.
Colours are the reference's tuples taken verbatim: element i goes to channel i of the frame.
"""
from __future__ import annotations

import torch

from . import geometry
from ._args import frame_clip

# vggt/vis/frame_visualization.py: the COCO-17 edges (a list of names, as the reference's)
COCO_SKELETON = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 7), (7, 9), (6, 8), (8, 10), (5, 6), (5, 11), (6, 12), (11, 12), (11, 13), (13, 15),
                 (12, 14), (14, 16)]
SKELETON_COLOUR = (0, 255, 255)
INDEX_COLOUR = (255, 255, 255)
TITLE_LEFT = "Left/Cam1 (Green=Observed, Red=Reprojected)"
TITLE_RIGHT = "Right/Cam2"


def keypoint_shapes(keypoints, *, color=(0, 255, 0), radius=4, thickness=-1, with_index=True, skeleton=COCO_SKELETON, scores=None,
                    score_thresh=None) -> torch.Tensor:
    """draw_keypoints' shape list: keypoints [..., K, >= 2] -> int32 [..., P, 8] with P = K + K digits + edges, digits =
    len(str(K - 1)) when with_index, in this order: the K points, the K index labels (`digits` records each), the edges.
    Plain torch ops on the keypoints' device."""
    kp = torch.as_tensor(keypoints)
    if kp.dim() < 2 or kp.shape[-1] < 2:
        raise ValueError(f"keypoints shape must be (..., K, >=2), got {list(kp.shape)}")
    kxy = kp[..., :2].to(torch.float64)
    K = int(kxy.shape[-2])
    mask = torch.ones(kxy.shape[:-1], dtype=torch.bool, device=kxy.device)
    if scores is not None and score_thresh is not None:
        sc = torch.as_tensor(scores, device=kxy.device)
        if sc.dim() == kxy.dim() and sc.shape[-1] == 1:
            sc = sc[..., 0]
        if sc.shape[-1] != K:
            raise ValueError(f"scores len {sc.shape[-1]} != keypoints K {K}")
        mask = (sc >= float(score_thresh)).expand(mask.shape)
    lists = [geometry.disc_shapes(kxy, radius, color, thickness, valid=mask)]
    if with_index and K:
        # the reference numbers the points that pass the score filter, in order: enumerate(kxy[mask])
        number = torch.cumsum(mask.to(torch.int64), dim=-1) - 1
        anchor = torch.round(kxy) + torch.tensor([4.0, -4.0], dtype=torch.float64, device=kxy.device)
        lists.append(geometry.number_shapes(number, anchor, len(str(K - 1)), 1, INDEX_COLOUR, valid=mask))
    if skeleton is not None:
        edges = [(int(i), int(j)) for i, j in skeleton if 0 <= int(i) < K and 0 <= int(j) < K]
        if edges:
            ia = torch.tensor([e[0] for e in edges], dtype=torch.int64, device=kxy.device)
            ib = torch.tensor([e[1] for e in edges], dtype=torch.int64, device=kxy.device)
            lists.append(geometry.segment_shapes(kxy.index_select(-2, ia), kxy.index_select(-2, ib), SKELETON_COLOUR, 2))
    return geometry.cat_shapes(*lists)


def draw_keypoints(frames, keypoints, *, color=(0, 255, 0), radius=4, thickness=-1, with_index=True, skeleton=COCO_SKELETON,
                   scores=None, score_thresh=None) -> torch.Tensor:
    """vggt/vis/frame_visualization.py: draw_and_save_keypoints_from_frame without the save, for a whole clip in one launch:
    frames uint8 [F, H, W, ch] or [C, F, H, W, ch], keypoints [F, K, >= 2] ([C, F, K, >= 2]; [K, >= 2]: the same points on every
    frame), device tensors -> the drawn frames (a new tensor).  The points first (cv2.circle: radius, thickness < 0 filled),
    then their indices (white, scale 1, at (+4, -4) of the rounded point), then the skeleton's edges (thickness 2), each
    edge only if both ends are finite.  scores [.., K] with score_thresh filter the POINTS and their labels only, and the
    labels count the points that pass, as the reference's enumerate over the filtered list; the edges are drawn from all
    finite joints.  A NaN joint is left out without a read-back: nothing is read back at all."""
    on = frame_clip("draw_keypoints", frames)[0].device
    kp = torch.as_tensor(keypoints)
    if not kp.is_cuda:
        raise geometry._lib.SkimiError("draw_keypoints needs device tensors (keypoints is on the host)")
    sh = keypoint_shapes(kp.to(on), color=color, radius=radius, thickness=thickness, with_index=with_index, skeleton=skeleton, scores=scores,
                         score_thresh=score_thresh)
    return geometry.draw_shapes(frames, sh)


# ---- the reprojection panel -----------------------------------------------------------------------------------------------
def reprojection_stats(kpt, proj) -> torch.Tensor:
    """kpt, proj [..., J, 2] -> float64 [..., 4] = RMSE, mean, median, max of the per-joint distances |proj - kpt|, NaN joints
    skipped (np.nanmean, np.nanmedian: the mean of the two middle values, np.nanmax), on the inputs' device; NaN without a
    finite joint."""
    d = torch.as_tensor(proj).to(torch.float64) - torch.as_tensor(kpt).to(torch.float64)
    err = torch.sqrt((d * d).sum(dim=-1))
    if err.shape[-1] == 0:
        return torch.full((*err.shape[:-1], 4), float("nan"), dtype=torch.float64, device=err.device)
    ok = ~torch.isnan(err)
    n = ok.sum(dim=-1)
    nf = n.to(torch.float64)
    z = torch.where(ok, err, torch.zeros_like(err))
    nan = torch.full_like(nf, float("nan"))
    rmse = torch.where(n > 0, torch.sqrt((z * z).sum(dim=-1) / nf), nan)
    mean = torch.where(n > 0, z.sum(dim=-1) / nf, nan)
    srt = torch.sort(torch.where(ok, err, torch.full_like(err, float("inf"))), dim=-1).values
    lo = ((n - 1).clamp(min=0) // 2)[..., None]
    hi = (n // 2).clamp(max=err.shape[-1] - 1)[..., None]
    med = torch.where(n > 0, (srt.gather(-1, lo)[..., 0] + srt.gather(-1, hi)[..., 0]) / 2.0, nan)
    mx = torch.where(n > 0, torch.where(ok, err, torch.full_like(err, float("-inf"))).amax(dim=-1), nan)
    return torch.stack([rmse, mean, med, mx], dim=-1)


def reprojection_shapes(obs, rep, width, height, joint_names=None, circle_r=5, thickness=2) -> torch.Tensor:
    """One view's list of render_reprojection_panel: obs, rep [..., J, 2] -> int32 [..., J (3 + L), 8], joint by joint as the
    reference draws: the observed point's green ring, the reprojected point's red ring (clipped to the frame as _clip_xy),
    the error vector (thickness 1), the label (L = the longest label's length; shorter ones are padded with kind 0).  A
    joint with a non-finite number in either point is left out."""
    o = torch.as_tensor(obs).to(torch.float64)
    r = torch.as_tensor(rep, device=o.device).to(torch.float64)
    J = int(o.shape[-2])
    hi = torch.tensor([float(width - 1), float(height - 1)], dtype=torch.float64, device=o.device)
    r = torch.minimum(torch.maximum(r, torch.zeros_like(hi)), hi)     # a NaN stays NaN, as np.clip's
    ok = torch.isfinite(o).all(dim=-1) & torch.isfinite(r).all(dim=-1)
    labels = [str(joint_names[j]) if joint_names is not None and j < len(joint_names) else str(j) for j in range(J)]
    L = max([len(s) for s in labels], default=0)
    ring_o = geometry.disc_shapes(o, circle_r, (0, 255, 0), thickness, valid=ok)[..., None, :]
    ring_r = geometry.disc_shapes(r, circle_r, (0, 0, 255), thickness, valid=ok)[..., None, :]
    line = geometry.segment_shapes(o, r, (255, 255, 0), 1, valid=ok)[..., None, :]
    codes = torch.from_numpy(geometry.string_codes(labels, L)).to(o.device)                      # [J, L]
    ro = torch.round(torch.where(ok[..., None], o, torch.zeros_like(o))).to(torch.int64)
    left = ro[..., 0, None] + 6 + torch.arange(L, dtype=torch.int64, device=o.device) * geometry.GLYPH_ADVANCE
    top = (ro[..., 1, None] - 6 - (geometry.GLYPH_HEIGHT - 1)).expand(left.shape)
    text = geometry.glyph_shapes(codes.expand(left.shape), left, top, 1, (0, 255, 0), valid=ok[..., None] & (codes >= 0))
    rec = torch.cat([ring_o, ring_r, line, text], dim=-2)                                        # [..., J, 3 + L, 8]
    return rec.reshape(*rec.shape[:-3], J * (3 + L), 8)


def _title_shapes(titles, x, y, scale, dev):
    """per-frame host strings -> int32 [len(titles), longest, 8] white glyphs from (x, y), text_shapes' bottom-left corner"""
    codes = torch.from_numpy(geometry.string_codes(titles)).to(dev)
    left = x + torch.arange(codes.shape[1], dtype=torch.int64, device=dev) * (geometry.GLYPH_ADVANCE * scale)
    top = torch.full_like(left, y - (geometry.GLYPH_HEIGHT * scale - 1))
    return geometry.glyph_shapes(codes, left.expand(codes.shape), top.expand(codes.shape), scale, (255, 255, 255), valid=codes >= 0)


def render_reprojection_panel(img1, img2, kptL, kptR, proj_L, proj_R, joint_names=None, circle_r=5, thickness=2, titles=True,
                              title_left=TITLE_LEFT, title_right=TITLE_RIGHT):
    """vggt/reproject.py: render_reprojection_panel for every frame of a clip at once: img1, img2 uint8 [F, H, W, ch] (the two
    views may differ in size, not in F or ch), kptL, kptR, proj_L, proj_R [F, J, 2], device tensors -> (visL, visR, panel): the
    two drawn views and the black panel [F, max(H1, H2), W1 + W2, ch] that holds them side by side.  Views of unequal height
    are placed top-aligned WITHOUT the reference's resize to a common height.  One launch per view and one for the titles.

    titles=True draws one title line per side with RMSE / mean / median / max of the side's reprojection errors.  The four
    numbers are computed on the device (reprojection_stats), but a title is a host string: THIS FUNCTION THEN READS BACK 8
    NUMBERS PER FRAME (one copy, one synchronisation).  titles=False draws no text on the panel and reads back nothing."""
    f1, five1 = frame_clip("render_reprojection_panel", img1)
    f2, five2 = frame_clip("render_reprojection_panel", img2)
    if five1 or five2 or f1.shape[1] != f2.shape[1] or f1.shape[4] != f2.shape[4]:
        raise ValueError(f"render_reprojection_panel: need two [F, H, W, ch] clips of one length and channel count, got {list(img1.shape)}, "
                         f"{list(img2.shape)}")
    dev = f1.device
    F, ch = int(f1.shape[1]), int(f1.shape[4])
    views, stats = [], []
    for fr, kpt, proj in ((f1[0], kptL, proj_L), (f2[0], kptR, proj_R)):
        k, p = torch.as_tensor(kpt), torch.as_tensor(proj)
        if not (k.is_cuda and p.is_cuda):
            raise geometry._lib.SkimiError("render_reprojection_panel needs device tensors")
        if k.dim() != 3 or k.shape[0] != F or k.shape[2] != 2 or p.shape != k.shape:
            raise ValueError(f"render_reprojection_panel: keypoints and reprojections must be [{F}, J, 2], got {list(k.shape)}, {list(p.shape)}")
        H, W = int(fr.shape[1]), int(fr.shape[2])
        views.append(geometry.draw_shapes(fr, reprojection_shapes(k.to(dev), p.to(dev), W, H, joint_names, circle_r, thickness)))
        stats.append(reprojection_stats(k.to(dev), p.to(dev)))
    visL, visR = views
    H1, W1, H2, W2 = int(visL.shape[1]), int(visL.shape[2]), int(visR.shape[1]), int(visR.shape[2])
    panel = torch.zeros((F, max(H1, H2), W1 + W2, ch), dtype=torch.uint8, device=dev)
    panel[:, :H1, :W1] = visL
    panel[:, :H2, W1:] = visR
    if titles and F:
        s = torch.stack(stats, dim=1).cpu().numpy()     # [F, 2, 4]: the one read-back
        line = "{} | RMSE={:.2f}px  (mean={:.2f}, med={:.2f}, max={:.2f})"
        left = _title_shapes([line.format(title_left, *s[f, 0]) for f in range(F)], 20, 30, 2, dev)
        right = _title_shapes([line.format(title_right, *s[f, 1]) for f in range(F)], W1 + 20, 30, 2, dev)
        geometry.draw_shapes(panel, geometry.cat_shapes(left, right), inplace=True)
    return visL, visR, panel


# ---- 3D scene views (geometry.render_scene, csrc/scene_view.hip) ------------------------------------------------------------
# vis_3d_kpt/visualization/scene_visualizer.py: the fixed box of draw_scene, the four views of draw_frame_with_scene and the
# matplotlib colours "r" (joints), "b" (links) and C0 (the origin marker), as RGB
SCENE_BOX = ((-0.5, 0.5), (-0.5, 0.5), (0.0, 1.8))
SCENE_PANEL_VIEWS = ((0, -90), (0, 90), (90, -90), (90, 90))
SCENE_PANEL_TITLES = ("Left view", "Right view", "left side view", "right side view", "top left view", "top right view")
SCENE_KPT_COLOUR, SCENE_LINK_COLOUR, SCENE_ORIGIN_COLOUR = (255, 0, 0), (0, 0, 255), (31, 119, 180)
SCENE_ORIGIN_LABEL = "world center (0,0,0)"
SCENE_BACKGROUND = (255, 255, 255)
# vggt/vis/vggt_camera_vis.py: the four views, the pad around the data, the cloud's grey
CAMERA_VIEWS = ((30, 60), (0, 90), (90, -90), (0, 0))
CAMERA_VIEW_NAMES = ("default", "front", "top", "side")
CAMERA_PAD = 0.05
CAMERA_POINT_GREY = 128


def scene_box_view(elev, azim, size, dev):
    """The orthographic view of draw_scene's box from (elev, azim) in matplotlib's convention: float64 [20] on dev.  The box's
    centre is the middle of the frame and its circumscribed sphere fits the frame's shorter side."""
    H, W = int(size[0]), int(size[1])
    centre = [sum(SCENE_BOX[0]) / 2, sum(SCENE_BOX[1]) / 2, sum(SCENE_BOX[2]) / 2]
    rad = sum(((hi - lo) / 2) ** 2 for lo, hi in SCENE_BOX) ** 0.5
    scale = min(H, W) / (2.1 * rad)
    return geometry.orbit_view(torch.tensor(centre, dtype=torch.float64, device=dev), 2.0 * rad, float(elev), float(azim), scale, scale, W / 2.0,
                               H / 2.0, 0.5 * rad, 3.5 * rad, ortho=True)


def draw_scene(kpts_world, skeleton=COCO_SKELETON, elev=0.0, azim=-90.0, size=(480, 480), label=True) -> torch.Tensor:
    """SceneVisualizer.draw_scene for a whole clip: kpts_world [T, J, 3] (or [J, 3]) device joints -> uint8 [T, H, W, 3] (RGB) on
    white: the floor grid of the reference's box (x, y in +-0.5, z in 0 .. 1.8; orthographic), the links, the joints and the
    origin marker, depth-tested, seen from (elev, azim); then, on top through the 2D rasteriser, the "world center (0,0,0)"
    label at the projected origin.  Nothing is read back."""
    k = torch.as_tensor(kpts_world)
    if not k.is_cuda:
        raise geometry._lib.SkimiError("draw_scene needs device tensors (kpts_world is on the host)")
    if k.dim() == 2:
        k = k[None]
    if k.dim() != 3 or k.shape[-1] != 3:
        raise ValueError(f"draw_scene: kpts_world must be [T, J, 3] or [J, 3], got {list(k.shape)}")
    dev, T = k.device, int(k.shape[0])
    view = scene_box_view(elev, azim, size, dev)
    origin = torch.zeros((1, 3), dtype=torch.float64, device=dev)
    prims = geometry.cat_prims(geometry.grid_prims("xy", 0.5, 0.25, view, (210, 210, 210)),
                               geometry.skeleton_prims(k, skeleton or [], view, SCENE_LINK_COLOUR, SCENE_KPT_COLOUR, 2.0, 3.0),
                               geometry.disc3d_prims(origin, view, SCENE_ORIGIN_COLOUR, 4.0))
    frames = geometry.render_scene(view[None].expand(T, -1).contiguous(), prims=prims, size=size, background=SCENE_BACKGROUND).frames
    if label and T:
        xy, _, ok = geometry.view_project(origin, view)
        offset = torch.tensor([6.0, -6.0], dtype=torch.float64, device=dev)
        geometry.draw_shapes(frames, geometry.text_shapes([SCENE_ORIGIN_LABEL], xy + offset, 1, (0, 0, 0), valid=ok), inplace=True)
    return frames


def fit_frames(frames, pane) -> torch.Tensor:
    """uint8 [T, H, W, 3] device frames -> [T, ph, pw, 3]: resized (preprocess.resize_bicubic_u8, aspect kept) to fit the pane and
    centred on white"""
    from . import preprocess
    ph, pw = int(pane[0]), int(pane[1])
    T, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    s = min(ph / H, pw / W)
    nh, nw = max(min(int(round(H * s)), ph), 1), max(min(int(round(W * s)), pw), 1)
    out = torch.full((T, ph, pw, 3), 255, dtype=torch.uint8, device=frames.device)
    y0, x0 = (ph - nh) // 2, (pw - nw) // 2
    for t in range(T):
        out[t, y0:y0 + nh, x0:x0 + nw] = preprocess.resize_bicubic_u8(frames[t], nw, nh)
    return out


def draw_frame_with_scene(left, right, pose_3d, skeleton=COCO_SKELETON, pane=(320, 320), titles=True) -> torch.Tensor:
    """SceneVisualizer.draw_frame_with_scene: left, right uint8 [T, H, W, 3] (or [H, W, 3]) device frames, pose_3d [T, J, 3] (or
    [J, 3]) -> the 2 x 3 panel uint8 [T, 2 ph, 3 pw, 3] (a single frame: [2 ph, 3 pw, 3]): row 0 = the left frame, the view
    (0, -90), the top view (90, -90); row 1 = the right frame, (0, 90), (90, 90).  The frames are fitted by fit_frames, the
    views are draw_scene's, the panes are assembled by device copies; titles=True writes the reference's six titles over
    the panes' top-left corners with the 2D rasteriser."""
    single = left.dim() == 3
    fl, fr = (left[None], right[None]) if single else (left, right)
    k = torch.as_tensor(pose_3d)
    k = k[None] if k.dim() == 2 else k
    fl, _ = frame_clip("draw_frame_with_scene", fl)
    fr, _ = frame_clip("draw_frame_with_scene", fr)
    T = int(fl.shape[1])
    if fl.shape[4] != 3 or fr.shape[4] != 3 or fr.shape[1] != T or k.shape[0] != T:
        raise ValueError(f"draw_frame_with_scene: need RGB clips and poses of one length, got {list(left.shape)}, {list(right.shape)}, "
                         f"{list(k.shape)}")
    ph, pw = int(pane[0]), int(pane[1])
    panel = torch.empty((T, 2 * ph, 3 * pw, 3), dtype=torch.uint8, device=fl.device)
    panel[:, :ph, :pw], panel[:, ph:, :pw] = fit_frames(fl[0], pane), fit_frames(fr[0], pane)
    for n, (el, az) in enumerate(SCENE_PANEL_VIEWS):
        r, c = n % 2, 1 + n // 2
        panel[:, r * ph:(r + 1) * ph, c * pw:(c + 1) * pw] = draw_scene(k, skeleton, el, az, pane)
    if titles and T:
        where = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
        anchors = torch.tensor([[c * pw + 6.0, r * ph + 14.0] for r, c in where], dtype=torch.float64, device=fl.device)
        geometry.draw_shapes(panel, geometry.text_shapes(list(SCENE_PANEL_TITLES), anchors, 1, (0, 0, 0)), inplace=True)
    return panel[0] if single else panel


def draw_camera_poses(extrinsic, points=None, center_mode="mean", intrinsic=None, colours=None, count=None, size=(400, 400), axis_len=0.1,
                      show_id=True) -> torch.Tensor:
    """vggt/vis/vggt_camera_vis.py: plot_cameras_from_predictions as a picture: extrinsic [S, 3, 4] device cameras, points [N, 3]
    (or any [..., 3]) world points or None -> uint8 [2 h, 2 w, 3] (RGB): the reference's four views (30, 60), (0, 90), (90, -90),
    (0, 0) in a 2 x 2 grid, each with every camera's three axes (x red, y green, z blue), its frustum (intrinsic [S, 3, 3];
    default: a unit-focal square image), its centre and its id, and the cloud splatted in grey, or in `colours` uint8 [N, 3].
    count: a device int64 scalar, the rows of points that exist.  center_mode "mean" | "first" | "none" moves the scene as
    the reference does.  The limits come from the camera centres and the finite points with the reference's 5 % pad,
    computed on the device; the views are orthographic with equal axes.  Nothing is read back."""
    E = torch.as_tensor(extrinsic)
    if not E.is_cuda:
        raise geometry._lib.SkimiError("draw_camera_poses needs device tensors (extrinsic is on the host)")
    if E.dim() != 3 or E.shape[-2:] != (3, 4):
        raise ValueError(f"draw_camera_poses: extrinsic must be [S, 3, 4], got {list(E.shape)}")
    dev, S = E.device, int(E.shape[0])
    E = E.to(torch.float64)
    C = geometry.camera_centres(E)
    if center_mode == "mean":
        centre = C.mean(dim=0)
    elif center_mode == "first":
        centre = C[0]
    elif center_mode == "none":
        centre = torch.zeros(3, dtype=torch.float64, device=dev)
    else:
        raise ValueError(f"Unknown center_mode: {center_mode}")
    lo, hi = (C - centre).amin(dim=0), (C - centre).amax(dim=0)
    xyz = rgb = None
    if points is not None and torch.as_tensor(points).numel():
        p = torch.as_tensor(points).to(dev).reshape(-1, 3)
        live = torch.isfinite(p).all(dim=-1)
        if count is not None:
            live = live & (torch.arange(p.shape[0], device=dev) < torch.as_tensor(count, device=dev).reshape(()))
        moved = p.to(torch.float64) - centre
        inf = torch.full_like(moved, float("inf"))
        lo = torch.minimum(lo, torch.where(live[:, None], moved, inf).amin(dim=0))
        hi = torch.maximum(hi, torch.where(live[:, None], moved, -inf).amax(dim=0))
        xyz = torch.where(live[:, None], moved, torch.full_like(moved, float("nan"))).to(torch.float32)[None]
        rgb = (torch.full((1, p.shape[0], 3), CAMERA_POINT_GREY, dtype=torch.uint8, device=dev) if colours is None
               else torch.as_tensor(colours).to(dev, torch.uint8).reshape(1, -1, 3))
    span = (hi - lo).amax().clamp(min=1e-9)
    half = 0.5 * span + CAMERA_PAD * span + axis_len        # the cube of the limits, and the markers that stick out of it
    mid = 0.5 * (lo + hi)
    h, w = int(size[0]), int(size[1])
    scale = min(h, w) / (2.0 * 3.0 ** 0.5 * half)           # the cube's circumscribed sphere fits the pane
    el = torch.tensor([v[0] for v in CAMERA_VIEWS], dtype=torch.float64, device=dev)
    az = torch.tensor([v[1] for v in CAMERA_VIEWS], dtype=torch.float64, device=dev)
    views = geometry.orbit_view(mid, 4.0 * half, el, az, scale, scale, w / 2.0, h / 2.0, 0.5 * half, 8.0 * half, ortho=True)
    K = (torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=dev).expand(S, 3, 3) if intrinsic is None
         else torch.as_tensor(intrinsic).to(dev, torch.float64))
    prims = geometry.cat_prims(geometry.camera_prims(E, K, views, axis_len, axis_len, offset=-centre),
                               geometry.disc3d_prims(C - centre, views, SCENE_ORIGIN_COLOUR, 3.0))
    panes = geometry.render_scene(views, xyz, rgb, prims=prims, size=(h, w), background=SCENE_BACKGROUND).frames
    corner = torch.tensor([6.0, 14.0], dtype=torch.float64, device=dev).expand(4, 4, 2)
    text = [geometry.text_shapes(list(CAMERA_VIEW_NAMES), corner, 1, (0, 0, 0), valid=torch.eye(4, dtype=torch.bool, device=dev))]
    if show_id and S:
        xy, _, ok = geometry.view_project(C - centre, views)                               # [4, S, 2]
        offset = torch.tensor([4.0, -4.0], dtype=torch.float64, device=dev)
        text.append(geometry.text_shapes([str(i) for i in range(S)], xy + offset, 1, (0, 0, 0), valid=ok))
    geometry.draw_shapes(panes, geometry.cat_shapes(*text), inplace=True)
    out = torch.empty((2 * h, 2 * w, 3), dtype=torch.uint8, device=dev)
    for n in range(4):
        out[(n // 2) * h:(n // 2 + 1) * h, (n % 2) * w:(n % 2 + 1) * w] = panes[n]
    return out
