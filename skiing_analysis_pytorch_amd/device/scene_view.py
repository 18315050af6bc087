"""3D scene views (csrc/scene_view.hip; C-ABI: skimi_scene_view_workspace_bytes, skimi_scene_view_render): the renderer's
wrapper, the view records and the builders of its depth-tested primitives; the reference's 3D pictures (draw.draw_scene,
draw.draw_frame_with_scene, draw.draw_camera_poses, bev.render_bev_skeleton_clip, infer.render_scene_views) are built on
these; rules: include/skimi.h, DESIGN §2 "Scene views".

render_scene is the one operation.  The builders are plain torch float64 ops on whatever device their inputs are on (so they
run in CPU tests) and never read back: a point that is NaN, or a segment wholly behind the near plane, becomes a record of
kind 0, which the kernel draws as nothing.  A view is float64 [..., 20]; a list is int32 [..., M, 12] under the views' leading
axes ([M, 12]: shared by every frame); lists are joined in drawing order with cat_prims.

Conventions.  A camera looks along its +z, x to the right and y DOWN (the VGGT / OpenCV frame), so v grows downwards.
Points land in the pixel (floor(u), floor(v)): pixel (i, j) covers [i, i + 1) x [j, j + 1).  A primitive's position is in
1/16 pixel with the centre of pixel (i, j) at (16 i, 16 j) as in draw_shapes, so the builders store round(16 (u - 0.5)): a
disc built at a point is centred on the pixel the point lands in.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from .._args import f32, i32, u8, workspace
from .._lib import check, current_stream, lib, ptr
from .draw import pack_colour

SCENE_MAX_PRIMS = 1024
SCENE_MAX_POINT_SIZE = 4
SCENE_NONE, SCENE_DISC, SCENE_CAPSULE = 0, 1, 2
SCENE_W_ONE = 1 << 30
SCENE_WORKSPACE_CAP = 256 << 20      # bytes of key buffer a call may hold: 16 frames of 1080p
VIEW_WORDS, PRIM_WORDS = 20, 12
_LIMIT = float(1 << 24)              # builders clamp positions here, inside int32; the kernel saturates to +-2^20 itself


class SceneView(NamedTuple):
    """render_scene's outputs (device tensors)."""
    frames: torch.Tensor             # uint8 [F, H, W, 3]
    depth: Optional[torch.Tensor]    # float32 [F, H, W]: Z of the winning fragment, +inf on an empty pixel; None unless asked
    index: Optional[torch.Tensor]    # int32 [F, H, W]: the nearest point's index, -1 where none landed; None unless asked


def _dev_tensor(fn, name, a, dtype, shape_ok, want):
    """a device tensor of `dtype` whose shape passes shape_ok, else ValueError (host tensors included)"""
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise ValueError(f"{fn}: {name} must be a device tensor (it is on {getattr(a, 'device', 'the host')})")
    if a.dtype != dtype:
        raise ValueError(f"{fn}: {name} must be {str(dtype).replace('torch.', '')}, got {a.dtype}")
    if not shape_ok(tuple(a.shape)):
        raise ValueError(f"{fn}: {name} must be {want}, got {list(a.shape)}")
    return a.contiguous()


def render_scene(views, xyz=None, rgb=None, count=None, cloud_of_frame=None, point_size=1, prims=None, size=None, background=0,
                 out=None, want_depth=False, want_index=False, workspace_cap=SCENE_WORKSPACE_CAP) -> SceneView:
    """Render F views of clouds and depth-tested primitives: views float64 [F, 20] (look_at_view, orbit_view,
    views_from_cameras), xyz float32 [P, N, 3] (or [N, 3]: one cloud) with rgb uint8 of the same shape (default: grey 160),
    count int64 [P] (the rows of each cloud that exist; the kernel reads it, the host does not), cloud_of_frame int32 [F]
    (default: cloud 0 when P == 1, the frame's index when P == F), point_size 1 .. 4, prims int32 [M, 12] or [F, M, 12] (M <=
    SCENE_MAX_PRIMS), all on the device -> SceneView.  background: a colour (one number or three) with size=(H, W), or uint8
    frames [F, H, W, 3] to draw over (not modified).  out: a preallocated uint8 [F, H, W, 3].  workspace_cap: the bytes of
    key buffer (8 a pixel) the call may hold; the frames are rendered in chunks that fit (at least one frame).  The number of
    launches depends on the shapes only; nothing is read back.  Rules: include/skimi.h."""
    fn = "render_scene"
    views = _dev_tensor(fn, "views", views, torch.float64, lambda s: len(s) == 2 and s[1] == VIEW_WORDS, "[F, 20]")
    dev, F = views.device, int(views.shape[0])
    if isinstance(background, torch.Tensor):
        bg = _dev_tensor(fn, "background", background, torch.uint8, lambda s: len(s) == 4 and s[0] == F and s[3] == 3, f"[{F}, H, W, 3]")
        H, W = int(bg.shape[1]), int(bg.shape[2])
        if size is not None and tuple(int(v) for v in size) != (H, W):
            raise ValueError(f"{fn}: size {tuple(size)} does not match the background frames {[H, W]}")
        colour = 0
    else:
        if size is None:
            raise ValueError(f"{fn}: size=(H, W) is needed with a background colour")
        bg, (H, W), colour = None, (int(v) for v in size), pack_colour(background)
    if H < 1 or W < 1:
        raise ValueError(f"{fn}: empty frame ({W} x {H})")
    P = N = 0
    if xyz is not None:
        if isinstance(xyz, torch.Tensor) and xyz.dim() == 2:
            xyz, rgb = xyz[None], (rgb[None] if isinstance(rgb, torch.Tensor) and rgb.dim() == 2 else rgb)
        xyz = _dev_tensor(fn, "xyz", xyz, torch.float32, lambda s: len(s) == 3 and s[2] == 3, "[P, N, 3]")
        P, N = int(xyz.shape[0]), int(xyz.shape[1])
        if rgb is None:
            rgb = torch.full((P, N, 3), 160, dtype=torch.uint8, device=dev)
        rgb = _dev_tensor(fn, "rgb", rgb, torch.uint8, lambda s: s == (P, N, 3), f"[{P}, {N}, 3]")
        if N >= 2 ** 31:
            raise ValueError(f"{fn}: a cloud holds at most 2^31 - 1 points, got {N}")
        if count is not None:
            count = _dev_tensor(fn, "count", count, torch.int64, lambda s: s == (P,), f"[{P}]")
        if cloud_of_frame is not None:
            cloud_of_frame = _dev_tensor(fn, "cloud_of_frame", cloud_of_frame, torch.int32, lambda s: s == (F,), f"[{F}]")
        elif P not in (1, F):
            raise ValueError(f"{fn}: {P} clouds for {F} frames need cloud_of_frame")
    elif rgb is not None or count is not None or cloud_of_frame is not None:
        raise ValueError(f"{fn}: rgb, count and cloud_of_frame need xyz")
    point_size = int(point_size)
    if not 1 <= point_size <= SCENE_MAX_POINT_SIZE:
        raise ValueError(f"{fn}: point_size must be 1 .. {SCENE_MAX_POINT_SIZE}, got {point_size}")
    M, axes = 0, 2
    if prims is not None:
        prims = _dev_tensor(fn, "prims", prims, torch.int32,
                            lambda s: len(s) in (2, 3) and s[-1] == PRIM_WORDS and (len(s) == 2 or s[0] == F), f"[M, 12] or [{F}, M, 12]")
        M, axes = int(prims.shape[-2]), prims.dim()
        if M > SCENE_MAX_PRIMS:
            raise ValueError(f"{fn}: {M} primitives in a list, at most {SCENE_MAX_PRIMS}")
    for name, a in (("xyz", xyz), ("rgb", rgb), ("count", count), ("cloud_of_frame", cloud_of_frame), ("prims", prims), ("background", bg)):
        if a is not None and a.device != dev:
            raise ValueError(f"{fn}: {name} is on {a.device}, views on {dev}")
    if out is None:
        frames = u8(dev, F, H, W, 3)
    else:
        frames = out
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != dev or out.dtype != torch.uint8
                or tuple(out.shape) != (F, H, W, 3) or not out.is_contiguous()):
            raise ValueError(f"{fn}: out must be a contiguous uint8 device tensor {[F, H, W, 3]}")
    depth = f32(dev, F, H, W) if want_depth else None
    index = i32(dev, F, H, W) if want_index else None
    if F == 0:
        return SceneView(frames, depth, index)
    ws = workspace(dev, lib().skimi_scene_view_workspace_bytes(F, H, W, max(int(workspace_cap), 1)))
    check(lib().skimi_scene_view_render(ptr(views), ptr(xyz), ptr(rgb), ptr(count), ptr(cloud_of_frame), P, N, point_size, ptr(prims),
                                        axes, M, ptr(bg), colour, ptr(frames), ptr(depth), ptr(index), F, H, W, ptr(ws), ws.numel(),
                                        current_stream()), "skimi_scene_view_render")
    return SceneView(frames, depth, index)


# ---- views ---------------------------------------------------------------------------------------------------------------
def host_const(values, dtype, dev):
    """Host numbers (a number, a list, a NumPy array) as a tensor of `dtype` on dev, without a synchronising copy: a single
    number is a fill on the device; an array goes through pinned memory and a non-blocking copy (torch's caching host
    allocator keeps the staging block alive until the copy has run).  On the host it is a plain tensor."""
    dev = torch.device(dev)
    a = np.asarray(values)
    if a.ndim == 0:
        return torch.full((), a.item(), dtype=dtype, device=dev)
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return t if dev.type == "cpu" else t.pin_memory().to(dev, non_blocking=True)


def _f64(a, dev=None):
    if isinstance(a, torch.Tensor):
        return a.to(device=a.device if dev is None else dev, dtype=torch.float64)
    return host_const(np.asarray(a, dtype=np.float64), torch.float64, "cpu" if dev is None else dev)


def _unit(v):
    return v / torch.sqrt((v * v).sum(dim=-1, keepdim=True))


def _record(R, t, fx, fy, cx, cy, near, far, ortho):
    """R [..., 3, 3], t [..., 3] and the seven numbers (numbers or tensors that broadcast to the leading axes) -> [..., 20]"""
    lead = R.shape[:-2]
    Rt = torch.cat([R, t[..., None]], dim=-1).reshape(*lead, 12)
    tail = [_f64(v, R.device).expand(lead) for v in (fx, fy, cx, cy, near, far, 1.0 if ortho else 0.0, 0.0)]
    return torch.cat([Rt, torch.stack(tail, dim=-1)], dim=-1).contiguous()


def look_at_view(eye, target, up, fx, fy, cx, cy, near, far, ortho=False) -> torch.Tensor:
    """The view of a camera at `eye` looking at `target`: eye, target, up [..., 3] -> float64 [..., 20].  forward = the unit
    vector eye -> target, right = unit(forward x up), down = forward x right; R's rows are right, down, forward and t = -R
    eye.  fx, fy: pixels per unit of X / Z (perspective) or per world unit (ortho)."""
    eye = _f64(eye)
    target, up = _f64(target, eye.device), _f64(up, eye.device)
    eye, target, up = torch.broadcast_tensors(eye, target, up)
    fwd = _unit(target - eye)
    right = _unit(torch.linalg.cross(fwd, up, dim=-1))
    down = torch.linalg.cross(fwd, right, dim=-1)
    R = torch.stack([right, down, fwd], dim=-2)
    t = -(R * eye[..., None, :]).sum(dim=-1)
    return _record(R, t, fx, fy, cx, cy, near, far, ortho)


def orbit_view(center, radius, elev_deg, azim_deg, fx, fy, cx, cy, near, far, ortho=False) -> torch.Tensor:
    """matplotlib's view_init as a view: the eye at center + radius (cos el cos az, cos el sin az, sin el) looking at center,
    world +z up.  center [..., 3]; elev_deg, azim_deg: numbers or tensors [...] -> float64 [..., 20].  At +-90 degrees
    elevation +z is the viewing axis; the up vector is then the horizontal direction that +z's image tends to as the
    elevation approaches, -sign(el) (cos az, sin az, 0) (at (90, -90): +y up, x to the right, as matplotlib's top view), so
    the top views are defined and continuous."""
    center = _f64(center)
    dev = center.device
    el, az = torch.deg2rad(_f64(elev_deg, dev)), torch.deg2rad(_f64(azim_deg, dev))
    ce, se, ca, sa = torch.cos(el), torch.sin(el), torch.cos(az), torch.sin(az)
    zero = torch.zeros_like(ce * ca)
    direction = torch.stack([ce * ca, ce * sa, se + zero], dim=-1)
    top = (ce.abs() < 1e-9)[..., None] & torch.ones_like(direction, dtype=torch.bool)
    sign = torch.where(se >= 0, -torch.ones_like(se), torch.ones_like(se))
    up = torch.where(top, torch.stack([sign * ca, sign * sa, zero], dim=-1), torch.stack([zero, zero, zero + 1.0], dim=-1))
    direction = torch.where(top, torch.stack([zero, zero, torch.sign(se) + zero], dim=-1), direction)
    return look_at_view(center + _f64(radius, dev)[..., None] * direction, center, up, fx, fy, cx, cy, near, far, ortho)


def views_from_cameras(extrinsic, intrinsic, near=0.01, far=1000.0) -> torch.Tensor:
    """The VGGT cameras as views: extrinsic [..., 3, 4] (world -> camera), intrinsic [..., 3, 3] -> float64 [..., 20] (fx, fy,
    cx, cy from K; its other entries are not part of the model)."""
    E = _f64(extrinsic)
    K = _f64(intrinsic, E.device)
    if E.shape[-2:] != (3, 4) or K.shape[-2:] != (3, 3):
        raise ValueError(f"views_from_cameras: need extrinsic [..., 3, 4] and intrinsic [..., 3, 3], got {list(E.shape)}, {list(K.shape)}")
    lead = torch.broadcast_shapes(E.shape[:-2], K.shape[:-2])
    E, K = E.expand(*lead, 3, 4), K.expand(*lead, 3, 3)
    return _record(E[..., :3], E[..., 3], K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], near, far, False)


def _to_camera(points, views):
    """points [..., n, 3] under views [..., 20] -> X, Y, Z [..., n] in rule 1's operation order, and the views as [..., 1, 20]"""
    p = _f64(points)
    V = _f64(views, p.device)
    if p.dim() < 2 or p.shape[-1] != 3 or V.dim() < 1 or V.shape[-1] != VIEW_WORDS:
        raise ValueError(f"need points [..., n, 3] and views [..., 20], got {list(p.shape)}, {list(V.shape)}")
    V = V[..., None, :]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    X = ((V[..., 0] * x + V[..., 1] * y) + V[..., 2] * z) + V[..., 3]
    Y = ((V[..., 4] * x + V[..., 5] * y) + V[..., 6] * z) + V[..., 7]
    Z = ((V[..., 8] * x + V[..., 9] * y) + V[..., 10] * z) + V[..., 11]
    return X, Y, Z, V


def _project_camera(X, Y, Z, V):
    """camera-frame points -> u, v float64, w int64 (clamped, a NaN gives 1), ok (rule 1's fragment test)"""
    near, far, ortho = V[..., 16], V[..., 17], V[..., 18] != 0
    ok = torch.isfinite(X) & torch.isfinite(Y) & torch.isfinite(Z) & (Z >= near) & (Z <= far) & (ortho | (Z > 0))
    Zs = torch.where(ortho | ~ok, torch.ones_like(Z), Z)
    u = torch.where(ortho, V[..., 12] * X + V[..., 14], (V[..., 12] * X) / Zs + V[..., 14])
    v = torch.where(ortho, V[..., 13] * Y + V[..., 15], (V[..., 13] * Y) / Zs + V[..., 15])
    q = torch.where(ortho, torch.floor((SCENE_W_ONE * (far - Z)) / (far - near)), torch.floor((SCENE_W_ONE * near) / Zs))
    q = torch.where(q >= 1.0, q, torch.ones_like(q)).clamp(max=float(SCENE_W_ONE))
    return u, v, q.to(torch.int64), ok


def view_project(points, views):
    """Project world points as the splat pass does: points [..., n, 3] under views [..., 20] (the leading axes broadcast) -> (xy
    float64 [..., n, 2] in pixels, w int32 [..., n], valid bool [..., n]).  valid is rule 1's fragment test (finite, near <= Z <=
    far, Z > 0 in a perspective view); xy and w of an invalid point are not meaningful.  The point's pixel is floor(xy)."""
    X, Y, Z, V = _to_camera(points, views)
    u, v, w, ok = _project_camera(X, Y, Z, V)
    return torch.stack([u, v], dim=-1), w.to(torch.int32), ok


# ---- primitives ----------------------------------------------------------------------------------------------------------
def _grid(u):
    """pixels -> int64 1/16 pixel of the primitives' grid: round(16 (u - 0.5)), non-finite -> 0"""
    u = torch.where(torch.isfinite(u), u, torch.zeros_like(u))
    return torch.round((u - 0.5) * 16.0).clamp(-_LIMIT, _LIMIT).to(torch.int64)


def _colour(colour, like):
    if isinstance(colour, torch.Tensor):      # packed colours already, broadcastable to the records
        return colour.to(like.device, torch.int64).expand(like.shape)
    return torch.full_like(like, pack_colour(colour))


def _prim_records(kind, x0, y0, x1, y1, r, colour, w0, w1, ok):
    """the nine words side by side and three zeros -> int32 [..., 12]; a record that is not ok is all zero (kind 0)"""
    full = lambda v: v.expand(x0.shape) if isinstance(v, torch.Tensor) else torch.full_like(x0, int(v))   # noqa: E731
    zero = torch.zeros_like(x0)
    rec = torch.stack([full(kind), x0, y0, full(x1), full(y1), full(r), _colour(colour, x0), full(w0), full(w1), zero, zero, zero], dim=-1)
    return torch.where(ok[..., None], rec, torch.zeros_like(rec)).to(torch.int32)


def _valid(valid, dev):
    return valid.to(dev, torch.bool) if isinstance(valid, torch.Tensor) else host_const(valid, torch.bool, dev)


def _length(v, like, scale):
    t = _f64(v, like.device)
    return torch.round(t * scale).clamp(0, _LIMIT).to(torch.int64).expand(like.shape)


def disc3d_prims(p, views, colour, radius_px=3.0, valid=None) -> torch.Tensor:
    """Discs of radius_px pixels at world points, at the points' depth: p [..., n, 3] under views [..., 20] -> int32 [..., n,
    12].  A point that is no fragment (view_project's valid), or valid == False, gives kind 0."""
    xy, w, ok = view_project(p, views)
    x0, y0 = _grid(xy[..., 0]), _grid(xy[..., 1])
    if valid is not None:
        ok = ok & _valid(valid, ok.device)
    w = w.to(torch.int64)
    return _prim_records(SCENE_DISC, x0, y0, x0, y0, _length(radius_px, x0, 16.0), colour, w, w, ok)


def clip_near(Xa, Ya, Za, Xb, Yb, Zb, near):
    """Clip the camera-frame segment a -> b against the plane Z = near: -> (Xa, Ya, Za, Xb, Yb, Zb, kept).  An end behind the
    plane moves to the plane along the segment (its Z becomes `near` exactly); a segment with both ends behind it (Z < near)
    is not kept; an end on the plane is in front."""
    a_in, b_in = Za >= near, Zb >= near
    dz = Zb - Za
    s = (near - Za) / torch.where(dz == 0, torch.ones_like(dz), dz)      # the crossing, used only where one end is behind
    Xc, Yc = Xa + s * (Xb - Xa), Ya + s * (Yb - Ya)
    move_a, move_b = ~a_in & b_in, a_in & ~b_in
    nz = near + torch.zeros_like(Za)
    return (torch.where(move_a, Xc, Xa), torch.where(move_a, Yc, Ya), torch.where(move_a, nz, Za),
            torch.where(move_b, Xc, Xb), torch.where(move_b, Yc, Yb), torch.where(move_b, nz, Zb), a_in | b_in)


def segment3d_prims(p0, p1, views, colour, thickness_px=2.0, valid=None) -> torch.Tensor:
    """Capsules between world points, thickness_px pixels wide, depth-interpolated between the ends: p0, p1 [..., n, 3] under
    views [..., 20] -> int32 [..., n, 12].  The segment is clipped against the near plane in 3D before projection
    (clip_near); a segment wholly behind it, with a non-finite end, with an end beyond `far` after the clip or (perspective)
    at Z <= 0, or valid == False, gives kind 0."""
    Xa, Ya, Za, V = _to_camera(p0, views)
    Xb, Yb, Zb, _ = _to_camera(p1, views)
    fin = torch.isfinite(Xa + Ya + Za + Xb + Yb + Zb)
    Xa, Ya, Za, Xb, Yb, Zb, kept = clip_near(Xa, Ya, Za, Xb, Yb, Zb, V[..., 16])
    ua, va, wa, oka = _project_camera(Xa, Ya, Za, V)
    ub, vb, wb, okb = _project_camera(Xb, Yb, Zb, V)
    ok = fin & kept & oka & okb
    if valid is not None:
        ok = ok & _valid(valid, ok.device)
    x0 = _grid(ua)
    return _prim_records(SCENE_CAPSULE, x0, _grid(va), _grid(ub), _grid(vb), _length(thickness_px, x0, 8.0), colour, wa, wb, ok)


def cat_prims(*lists) -> torch.Tensor:
    """lists in drawing order -> one list [..., M, 12]; a list with fewer leading axes is repeated under the others' axes"""
    lists = [x for x in lists if x is not None]
    lead = torch.broadcast_shapes(*[tuple(x.shape[:-2]) for x in lists])
    return torch.cat([x.expand(*lead, *x.shape[-2:]) for x in lists], dim=-2).contiguous()


def skeleton_prims(joints, links, views, bone_colour=(0, 0, 255), joint_colour=(255, 0, 0), thickness_px=2.0, radius_px=3.0) -> torch.Tensor:
    """A skeleton per view: joints [..., J, 3] under views [..., 20], links: host pairs of joint indices -> int32 [..., E + J,
    12]: the bones (capsules), then the joints (discs).  A NaN joint drops itself and its bones."""
    j = _f64(joints)
    J = int(j.shape[-2])
    edges = [(int(a), int(b)) for a, b in links if 0 <= int(a) < J and 0 <= int(b) < J]
    lists = []
    if edges:
        ia = host_const([e[0] for e in edges], torch.int64, j.device)
        ib = host_const([e[1] for e in edges], torch.int64, j.device)
        lists.append(segment3d_prims(j.index_select(-2, ia), j.index_select(-2, ib), views, bone_colour, thickness_px))
    lists.append(disc3d_prims(j, views, joint_colour, radius_px))
    return cat_prims(*lists)


CAMERA_AXIS_COLOURS = ((255, 0, 0), (0, 255, 0), (0, 0, 255))     # vggt_camera_vis.py: "r", "g", "b" for the camera's x, y, z
CAMERA_PRIMS_PER_CAMERA = 11


def camera_centres(extrinsic) -> torch.Tensor:
    """extrinsic [..., 3, 4] -> the cameras' centres -R^T t, float64 [..., 3]"""
    E = _f64(extrinsic)
    return -(E[..., :3].transpose(-1, -2) @ E[..., 3:4])[..., 0]


def camera_prims(extrinsic, intrinsic, views, axis_len=0.1, frustum_depth=0.1, frustum_colour=(64, 64, 64), thickness_px=1.0,
                 offset=None) -> torch.Tensor:
    """Camera markers: extrinsic [C, 3, 4], intrinsic [C, 3, 3] (the image is taken as 2 cx x 2 cy pixels) under views [..., 20]
    -> int32 [..., 11 C, 12]: per camera its three axes of axis_len (vggt_camera_vis.py: x red, y green, z blue), then a
    frustum of frustum_depth: the four edges from the centre to the image corners and the rectangle that joins them.
    offset [3]: added to every point (the reference's center_mode shift, negated)."""
    E = _f64(extrinsic)
    K = _f64(intrinsic, E.device)
    if E.dim() != 3 or E.shape[-2:] != (3, 4) or tuple(K.shape) != (E.shape[0], 3, 3):
        raise ValueError(f"camera_prims: need extrinsic [C, 3, 4] and intrinsic [C, 3, 3], got {list(E.shape)}, {list(K.shape)}")
    Rt = E[:, :, :3].transpose(1, 2)                       # columns: the camera's axes in the world
    centre = camera_centres(E)
    if offset is not None:
        centre = centre + _f64(offset, E.device)
    tips = centre[:, None, :] + axis_len * Rt.transpose(1, 2)                 # [C, 3 axes, 3]
    fx, fy, cx, cy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    sx, sy = host_const([-1.0, 1.0, 1.0, -1.0], torch.float64, E.device), host_const([-1.0, -1.0, 1.0, 1.0], torch.float64, E.device)
    corner_cam = torch.stack([sx * (cx / fx)[:, None], sy * (cy / fy)[:, None], torch.ones_like(sx).expand(E.shape[0], 4)], dim=-1)
    corners = centre[:, None, :] + (frustum_depth * corner_cam) @ Rt.transpose(1, 2)     # [C, 4, 3]
    c3, c4 = centre[:, None, :].expand(-1, 3, -1), centre[:, None, :].expand(-1, 4, -1)
    a = torch.cat([c3, c4, corners], dim=1).reshape(-1, 3)                    # [11 C, 3]
    b = torch.cat([tips, corners, corners.roll(-1, dims=1)], dim=1).reshape(-1, 3)
    axis = host_const([pack_colour(c) for c in CAMERA_AXIS_COLOURS] + [pack_colour(frustum_colour)] * 8, torch.int64, E.device).repeat(E.shape[0])
    return segment3d_prims(a, b, views, axis, thickness_px)


def grid_prims(plane, extent, step, views, colour=(200, 200, 200), thickness_px=1.0, level=0.0, origin=(0.0, 0.0)) -> torch.Tensor:
    """Grid lines on a coordinate plane: plane "xy", "xz" or "yz" at `level` on the third axis, lines every `step` from
    -extent to +extent around `origin` (extent a number, or (extent_a, extent_b) for the plane's two axes) under views [...,
    20] -> int32 [..., M, 12].  The line positions are host numbers."""
    axes = {"xy": (0, 1, 2), "xz": (0, 2, 1), "yz": (1, 2, 0)}.get(plane)
    if axes is None or not step > 0:
        raise ValueError(f"grid_prims: plane must be 'xy', 'xz' or 'yz' and step > 0, got {plane!r}, {step}")
    ea, eb = (float(extent), float(extent)) if np.isscalar(extent) else (float(extent[0]), float(extent[1]))
    ta = np.arange(-math.floor(ea / step + 1e-9), math.floor(ea / step + 1e-9) + 1) * float(step)
    tb = np.arange(-math.floor(eb / step + 1e-9), math.floor(eb / step + 1e-9) + 1) * float(step)
    a = np.full((len(ta) + len(tb), 3), float(level))
    b = a.copy()
    a[:len(ta), axes[0]], b[:len(ta), axes[0]] = origin[0] + ta, origin[0] + ta          # lines along the second axis
    a[:len(ta), axes[1]], b[:len(ta), axes[1]] = origin[1] - eb, origin[1] + eb
    a[len(ta):, axes[1]], b[len(ta):, axes[1]] = origin[1] + tb, origin[1] + tb          # lines along the first
    a[len(ta):, axes[0]], b[len(ta):, axes[0]] = origin[0] - ea, origin[0] + ea
    dev = torch.as_tensor(views).device
    return segment3d_prims(host_const(a, torch.float64, dev), host_const(b, torch.float64, dev), views, colour, thickness_px)
