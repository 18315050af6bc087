"""GPU: the scene-view renderer (csrc/scene_view.hip) against the NumPy restatement (tests/scene_view_restated.py): frames and
index byte for byte, depth bit for bit, every call run twice and compared with itself, the inputs checked untouched; and the
reference-named functions on top of it."""
import functools

import numpy as np
import pytest
import torch

import scene_view_cases as sc
import scene_view_restated as sr
from skiing_analysis_pytorch_amd import _lib, bev, draw, geometry, infer

pytestmark = pytest.mark.gpu


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def cloud(P, N=sc.N_POINTS, seed=0):
    return sc.cloud(P, N, seed)


def check(views, xyz=None, rgb=None, count=None, cof=None, point_size=1, prims=None, size=None, background=0, **kw):
    """render on the device, twice: equal to the restatement, the rerun bitwise identical, the inputs untouched"""
    H, W = size
    host = [a for a in (views, xyz, rgb, count, cof, prims, background if isinstance(background, np.ndarray) else None)]
    dv = [dev(a) for a in host]
    keep = [None if a is None else a.clone() for a in dv]
    cnt = None if count is None else dv[3].to(torch.int64)
    cf = None if cof is None else dv[4].to(torch.int32)
    bg = dv[6] if isinstance(background, np.ndarray) else background
    call = lambda: geometry.render_scene(dv[0], dv[1], dv[2], count=cnt, cloud_of_frame=cf, point_size=point_size, prims=dv[5], size=(H, W),   # noqa: E731
                                         background=bg, want_depth=True, want_index=True, **kw)
    got, again = call(), call()
    F = len(views)
    assert got.frames.dtype == torch.uint8 and tuple(got.frames.shape) == (F, H, W, 3)
    assert got.depth.dtype == torch.float32 and tuple(got.depth.shape) == (F, H, W)
    assert got.index.dtype == torch.int32 and tuple(got.index.shape) == (F, H, W)
    for a, b in zip(dv, keep):
        assert a is None or a.numel() == 0 or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
    wf, wd, wi = sr.render(views, xyz, rgb, count, cof, point_size, prims, H, W, background)
    g = got.frames.cpu().numpy()
    bad = np.argwhere(g != wf)
    assert not len(bad), f"{len(bad)} bytes differ from the restatement, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {wf[tuple(bad[0])]}"
    assert (got.index.cpu().numpy() == wi).all()
    assert (got.depth.cpu().numpy().view(np.uint32) == wd.view(np.uint32)).all()
    assert torch.equal(got.frames, again.frames) and torch.equal(got.index, again.index)
    assert torch.equal(got.depth.view(torch.int32), again.depth.view(torch.int32))
    return got, (wf, wd, wi)


# ---- splat ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ortho", [False, True])
@pytest.mark.parametrize("point_size", [1, 3])
@pytest.mark.parametrize("size,F", [(sc.SIZES[0], 1), (sc.SIZES[1], 3)])
def test_splat_equals_restatement(size, F, point_size, ortho):
    xyz, rgb = cloud(1)                                   # one cloud shared by every frame
    got, (wf, _, wi) = check(sc.views(F, *size, ortho), xyz, rgb, point_size=point_size, size=size, background=(1, 2, 3))
    assert (wi >= 0).any() and (wf != [1, 2, 3]).any()


def test_count_hides_the_rows_behind_it():
    H, W = sc.SIZES[1]
    xyz, rgb = (a.copy() for a in cloud(1))
    n = 3100
    xyz[:, n:n + 600] = np.nan
    xyz[:, n + 600:] = np.float32(3e38)
    xyz[:, n + 900:, 0] = np.float32(1.0)                  # in front of the cameras, if it were read
    vs = sc.views(3, H, W)
    with_count, _ = check(vs, xyz, rgb, count=np.array([n]), point_size=3, size=(H, W))
    cut, _ = check(vs, xyz[:, :n], rgb[:, :n], point_size=3, size=(H, W))
    assert torch.equal(with_count.frames, cut.frames) and torch.equal(with_count.index, cut.index)
    assert torch.equal(with_count.depth.view(torch.int32), cut.depth.view(torch.int32))
    check(vs[:1], xyz, rgb, count=np.array([0]), size=(H, W))
    check(vs[:1], xyz, rgb, count=np.array([-7]), size=(H, W))
    check(vs[:1], xyz, rgb, count=np.array([10 ** 12]), size=(H, W))          # clipped to N


def test_cloud_per_frame_and_explicit_assignment():
    H, W = sc.SIZES[1]
    xyz, rgb = cloud(3, 1500, 2)
    vs = sc.views(3, H, W)
    per_frame, _ = check(vs, xyz, rgb, count=np.array([1500, 900, 1200]), size=(H, W))              # P == F
    picked, _ = check(vs, xyz, rgb, count=np.array([1500, 900, 1200]), cof=np.array([2, 2, 0]), size=(H, W))
    assert not torch.equal(per_frame.frames, picked.frames)
    alone, _ = check(vs[1:2], xyz[2:3], rgb[2:3], count=np.array([1200]), size=(H, W))
    assert torch.equal(alone.frames[0], picked.frames[1]) and torch.equal(alone.index[0], picked.index[1])
    check(vs, xyz, rgb, cof=np.array([1, -1, 3]), size=(H, W))                                     # outside 0 .. P - 1: no cloud


def test_no_points_and_no_cloud():
    H, W = sc.SIZES[0]
    vs = sc.views(1, H, W)
    for kw in (dict(xyz=np.zeros((1, 0, 3), dtype=np.float32), rgb=np.zeros((1, 0, 3), dtype=np.uint8)), dict()):
        got, _ = check(vs, size=(H, W), background=(7, 8, 9), **kw)
        assert (got.index == -1).all() and torch.isinf(got.depth).all()
        assert (got.frames.cpu().numpy() == [7, 8, 9]).all()


# ---- primitives ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,F", [(sc.SIZES[0], 1), (sc.SIZES[1], 3)])
@pytest.mark.parametrize("M", sc.COUNTS)
def test_list_lengths(M, size, F):
    H, W = size
    xyz, rgb = cloud(1, 1500, 2)
    check(sc.views(F, H, W), xyz, rgb, prims=sc.counted(M, H, W), size=size, background=40)


def test_300_primitives_on_one_tile():
    H, W = sc.SIZES[1]
    got, (wf, _, _) = check(sc.views(1, H, W), prims=sc.one_tile(300), size=(H, W))
    assert wf[0, :16, :64].any() and not wf[0, 40:].any()


@pytest.mark.parametrize("axes", ["shared", "per_frame"])
def test_list_layouts(axes):
    H, W = sc.SIZES[1]
    xyz, rgb = cloud(1)
    prims = sc.random_prims(64, H, W, 5) if axes == "shared" else np.stack([sc.random_prims(64, H, W, 20 + f) for f in range(3)])
    got, _ = check(sc.views(3, H, W, ortho=True), xyz, rgb, prims=prims, point_size=2, size=(H, W))
    if axes == "per_frame":
        d = [dev(a) for a in (sc.views(3, H, W, ortho=True)[2:3], xyz, rgb, prims[2])]
        alone = geometry.render_scene(d[0], d[1], d[2], point_size=2, prims=d[3], size=(H, W))
        assert torch.equal(alone.frames[0], got.frames[2])


@pytest.mark.parametrize("size", sc.SIZES)
def test_special_primitives(size):
    H, W = size
    xyz, rgb = cloud(1, 1500, 2)
    check(sc.views(1, H, W), xyz, rgb, prims=sc.special_prims(H, W), size=size)
    got, (wf, wd, _) = check(sc.views(1, H, W), prims=sc.special_prims(H, W), size=size)
    assert np.isfinite(wd).all()                            # the disc larger than the frame is behind everything
    assert (wf[0, 6, 31] == [0x21, 0x43, 0x65]).all()       # equal w: the later primitive


@pytest.mark.parametrize("ortho", [False, True])
@pytest.mark.parametrize("size", sc.SIZES)
def test_capsule_through_a_plane_of_points_and_equal_w(size, ortho):
    H, W = size
    v, xyz, rgb, prims, wp = sc.plane_case(H, W, ortho)
    got, (wf, _, wi) = check(v, xyz, rgb, prims=prims, size=size)
    wm, pt = sr.fragment_map(prims[0], H, W), wi[0] >= 0
    f = got.frames[0].cpu().numpy()
    assert ((wm > wp) & pt).any() and ((wm > 0) & (wm < wp) & pt).any()
    assert (f[(wm > wp) & pt] == [255, 0, 255]).all() and not (f[(wm > 0) & (wm < wp) & pt] == [255, 0, 255]).all(axis=-1).any()
    d0 = (sr.fragment_map(prims[1], H, W) > 0) & pt & (wm <= wp)
    assert d0.any() and (f[d0] == [0, 255, 0]).all()        # the disc of the plane's own w beats the points


# ---- the other arguments ---------------------------------------------------------------------------------------------------
def test_identity_case():
    view, xyz, rgb, (H, W) = sc.identity_case()
    got, _ = check(view, xyz, rgb, size=(H, W))
    assert (got.index[0].reshape(-1).cpu().numpy() == np.arange(H * W)).all()
    assert (got.frames[0].reshape(-1, 3).cpu().numpy() == rgb[0]).all()


def test_background_frames_and_out():
    H, W = sc.SIZES[1]
    xyz, rgb = cloud(1, 1500, 2)
    vs, prims = sc.views(3, H, W), sc.random_prims(64, H, W, 8)
    bg = np.random.default_rng(1).integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    got, (wf, _, wi) = check(vs, xyz, rgb, prims=prims, size=(H, W), background=bg)
    assert (wf == bg).any() and (wf != bg).any()
    out = torch.full((3, H, W, 3), 9, dtype=torch.uint8, device="cuda")
    res = geometry.render_scene(dev(vs), dev(xyz), dev(rgb), prims=dev(prims), background=dev(bg), out=out)
    assert res.frames.data_ptr() == out.data_ptr() and torch.equal(out, got.frames) and res.depth is None and res.index is None
    one = geometry.render_scene(dev(vs), dev(xyz[0]), dev(rgb[0]), prims=dev(prims), background=dev(bg))     # [N, 3]: one cloud
    assert torch.equal(one.frames, got.frames)


@pytest.mark.parametrize("F", [1, 3])
def test_dword_aligned_rows(F):
    """40 x 72 and 24 x 132: 3 W is a multiple of 4, so the resolve pass loads the background and stores the frame as dwords;
    the second size has a ragged last span (132 = 33 spans) and more than one tile across"""
    xyz, rgb = cloud(1, 1500, 2)
    for k, (H, W) in enumerate(((40, 72), (24, 132))):
        vs = sc.views(F, H, W, ortho=bool(k))
        prims = np.concatenate([sc.special_prims(H, W)[1:], sc.random_prims(24, H, W, 40 + k)])     # without the disc that covers the frame
        bg = np.random.default_rng(5 + k).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
        got, (wf, _, wi) = check(vs, xyz, rgb, prims=prims, size=(H, W), background=bg)
        assert (wf == bg).all(axis=-1).any() and (wi >= 0).any()
        check(vs, xyz, rgb, prims=prims, size=(H, W), background=(250, 3, 77))


def test_chunked_equals_unchunked():
    H, W = sc.SIZES[1]
    xyz, rgb = cloud(3, 1500, 2)
    vs = sc.views(3, H, W)
    prims = np.stack([sc.random_prims(64, H, W, 30 + f) for f in range(3)])
    bg = np.random.default_rng(2).integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    whole, _ = check(vs, xyz, rgb, count=np.array([1500, 900, 1200]), prims=prims, size=(H, W), background=bg)
    for cap in (1, 8 * H * W, 2 * 8 * H * W + 5):           # one frame, one frame, two frames at a time
        part, _ = check(vs, xyz, rgb, count=np.array([1500, 900, 1200]), prims=prims, size=(H, W), background=bg, workspace_cap=cap)
        assert torch.equal(part.frames, whole.frames) and torch.equal(part.index, whole.index)
        assert torch.equal(part.depth.view(torch.int32), whole.depth.view(torch.int32))
    lib = _lib.lib()
    assert lib.skimi_scene_view_workspace_bytes(3, H, W, 0) == 3 * 8 * H * W
    assert lib.skimi_scene_view_workspace_bytes(3, H, W, 1) == 8 * H * W
    assert lib.skimi_scene_view_workspace_bytes(3, H, W, 2 * 8 * H * W + 5) == 2 * 8 * H * W


def test_builders_on_the_device_feed_the_renderer():
    """the records built on the device are the ones built on the host to one grid unit (two correctly rounded evaluations may
    differ where a value sits on a rounding boundary), and the picture is the restatement's of the device's records"""
    H, W = sc.SIZES[1]
    vs = sc.views(3, H, W)
    j = sc.skeleton_clip(3)
    links = draw.COCO_SKELETON
    E = np.stack([v[:12].reshape(3, 4) for v in sc.views(2, H, W)])
    K = np.array([[[60.0, 0, 30], [0, 60.0, 20], [0, 0, 1]]] * 2)
    build = lambda t: geometry.cat_prims(geometry.grid_prims("xy", 1.0, 0.5, t(vs)), geometry.skeleton_prims(t(j) - t(np.array([0, 0, 0.8])), links, t(vs)),   # noqa: E731
                                         geometry.camera_prims(t(E), t(K), t(vs), 0.3, 0.4))
    on_dev, on_host = build(dev), build(torch.from_numpy)
    diff = (on_dev.cpu().long() - on_host.long()).abs()
    assert on_dev.is_cuda and on_dev.shape == on_host.shape and diff[..., [0, 5, 6]].max() == 0 and diff.max() <= 1
    xyz, rgb = cloud(1, 1500, 2)
    got, (wf, _, _) = check(vs, xyz, rgb, prims=on_dev.cpu().numpy(), size=(H, W), background=255)
    assert (wf != 255).any()


# ---- the reference's functions ---------------------------------------------------------------------------------------------
def test_draw_scene_and_frame_with_scene():
    T, pane = 2, (90, 110)
    j = dev(sc.skeleton_clip(T))
    left = dev(np.random.default_rng(3).integers(0, 256, size=(T, 48, 80, 3), dtype=np.uint8))
    right = dev(np.random.default_rng(4).integers(0, 256, size=(T, 70, 50, 3), dtype=np.uint8))
    panel = draw.draw_frame_with_scene(left, right, j, pane=pane, titles=False)
    ph, pw = pane
    assert tuple(panel.shape) == (T, 2 * ph, 3 * pw, 3) and panel.dtype == torch.uint8
    assert torch.equal(panel[:, :ph, :pw], draw.fit_frames(left, pane)) and torch.equal(panel[:, ph:, :pw], draw.fit_frames(right, pane))
    for n, (el, az) in enumerate(draw.SCENE_PANEL_VIEWS):
        view = draw.draw_scene(j, elev=el, azim=az, size=pane)
        r, c = n % 2, 1 + n // 2
        assert torch.equal(panel[:, r * ph:(r + 1) * ph, c * pw:(c + 1) * pw], view)
        assert (view != 255).any(dim=-1).sum() > 100 and not torch.equal(view[0], view[1])
        # the picture is the restatement's of the same records, then the label through the 2D rasteriser
        bare = draw.draw_scene(j, elev=el, azim=az, size=pane, label=False)
        v = draw.scene_box_view(el, az, pane, "cuda")
        prims = geometry.cat_prims(geometry.grid_prims("xy", 0.5, 0.25, v, (210, 210, 210)),
                                   geometry.skeleton_prims(j, draw.COCO_SKELETON, v, draw.SCENE_LINK_COLOUR, draw.SCENE_KPT_COLOUR, 2.0, 3.0),
                                   geometry.disc3d_prims(torch.zeros(1, 3, dtype=torch.float64, device="cuda"), v, draw.SCENE_ORIGIN_COLOUR, 4.0))
        want, _, _ = sr.render(v[None].expand(T, -1).cpu().numpy(), None, None, None, None, 1, prims.cpu().numpy(), ph, pw, (255, 255, 255))
        assert (bare.cpu().numpy() == want).all() and not torch.equal(bare, view)
    titled = draw.draw_frame_with_scene(left, right, j, pane=pane)
    assert not torch.equal(titled, panel) and torch.equal(titled[:, 20:ph], panel[:, 20:ph])
    single = draw.draw_frame_with_scene(left[0], right[0], j[0], pane=pane, titles=False)
    assert torch.equal(single, panel[0])


def test_draw_camera_poses_and_bev_clip():
    H, W = sc.SIZES[1]
    E = dev(np.stack([v[:12].reshape(3, 4) for v in sc.views(3, H, W)]))
    xyz, _ = cloud(1, 1500, 2)
    h, w = 96, 120
    for kw in (dict(), dict(points=dev(xyz[0])), dict(points=dev(xyz[0]), center_mode="first", count=torch.tensor(700, device="cuda")),
               dict(points=dev(xyz[0]), colours=dev(cloud(1, 1500, 2)[1][0]), center_mode="none")):
        img = draw.draw_camera_poses(E, size=(h, w), axis_len=0.4, **kw)
        assert tuple(img.shape) == (2 * h, 2 * w, 3) and img.dtype == torch.uint8
        for n in range(4):
            pane = img[(n // 2) * h:(n // 2 + 1) * h, (n % 2) * w:(n % 2 + 1) * w]
            assert (pane[20:] != 255).any(dim=-1).sum() > 30, (kw.keys(), n)
    with pytest.raises(ValueError):
        draw.draw_camera_poses(E, center_mode="median")
    T = 3
    k = np.zeros((T, 17, 3))
    rng = np.random.default_rng(6)
    k[..., 0], k[..., 1], k[..., 2] = rng.uniform(-6, 6, (T, 17)), rng.uniform(0, 1.8, (T, 17)), rng.uniform(4, 16, (T, 17))
    clip = bev.render_bev_skeleton_clip(dev(k), size=(90, 160))
    assert tuple(clip.shape) == (T, 90, 160, 3) and clip.dtype == torch.uint8
    green = (clip == torch.tensor([0, 255, 0], dtype=torch.uint8, device="cuda")).all(dim=-1)
    assert (green.reshape(T, -1).sum(dim=1) > 50).all() and not torch.equal(clip[0], clip[1])
    assert tuple(bev.render_bev_skeleton_clip(dev(k[:1])).shape) == (1, 720, 1280, 3)


def test_render_scene_views_reads_nothing_back():
    """a small synthetic scene through geometry.scene_point_cloud, rendered from its own cameras and from an orbit with
    torch's sync debug mode at "error" (the idiom of tests/test_person_gpu.py): no call on the path may synchronise, the
    builders' uploads of host constants included"""
    B, S, H, W = 1, 2, 20, 28
    rng = np.random.default_rng(8)
    K = np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]])
    E = np.stack([np.eye(4)[:3], np.eye(4)[:3]])
    E[1, 0, 3] = -0.3
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    pts = []
    for s in range(S):
        d = rng.uniform(2.0, 3.0, (H, W))
        cam = np.stack([(u - K[0, 2]) / 30.0 * d, (v - K[1, 2]) / 30.0 * d, d], axis=-1)
        pts.append(cam - E[s, :, 3])
    points = dev(np.stack(pts)[None].astype(np.float32))
    conf = dev(rng.uniform(1, 2, (B, S, H, W)).astype(np.float32))
    images = dev(rng.uniform(0, 1, (B, S, 3, H, W)).astype(np.float32))
    Ed, Kd = dev(E), dev(np.stack([K, K]))
    sc_cloud = geometry.scene_point_cloud(points, conf, images, Ed[None].float(), conf_thres=30.0)
    joints = dev(np.array([[0.0, 0.0, 2.0], [0.2, 0.1, 2.0], [0.2, 0.4, 2.2]]))
    kw = dict(joints=joints, links=[(0, 1), (1, 2)], size=(H, W), want_index=True)
    infer.render_scene_views(sc_cloud, Ed, Kd, **kw)          # sizes the allocator's pools
    infer.render_scene_views(sc_cloud, Ed, Kd, orbit=(5, 20.0), **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        own = infer.render_scene_views(sc_cloud, Ed, Kd, **kw)
        orbit = infer.render_scene_views(sc_cloud, Ed, Kd, orbit=(5, 20.0), image_size=(H, W), **kw)
        with pytest.raises(RuntimeError):
            own.frames.cpu()                                  # the mode is armed: a read-back raises
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(own.frames.shape) == (S, H, W, 3) and tuple(orbit.frames.shape) == (5, H, W, 3)
    n = int(sc_cloud.count[0])
    assert 0 < n < S * H * W
    # from its own first camera the kept pixels of view 0 land where they came from
    seen = own.index[0].cpu().numpy()
    assert (seen >= 0).sum() > 0.5 * H * W and seen.max() < n
    for f in range(5):
        assert (orbit.index[f] >= 0).any() and (orbit.frames[f] != 255).any()


# ---- error paths -----------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_bad_arguments():
    H, W = sc.SIZES[0]
    vs, (xyz, rgb) = dev(sc.views(2, H, W)), (dev(a) for a in cloud(1, 1500, 2))
    ok = dict(views=vs, xyz=xyz, rgb=rgb, size=(H, W))
    geometry.render_scene(**ok)
    zeros = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")   # noqa: E731
    for change in (dict(views=vs.cpu()), dict(xyz=xyz.cpu()), dict(views=vs.float()), dict(xyz=xyz.double()), dict(rgb=rgb.int()),
                   dict(views=vs[:, :19]), dict(rgb=rgb[:, :10]), dict(prims=zeros(geometry.SCENE_MAX_PRIMS + 1, 12)), dict(prims=zeros(4, 8)),
                   dict(prims=zeros(3, 4, 12)), dict(prims=zeros(4, 12).long()), dict(point_size=0), dict(point_size=5), dict(size=None),
                   dict(size=(0, W)), dict(count=torch.zeros(1, dtype=torch.int32, device="cuda")), dict(count=torch.zeros(2, dtype=torch.int64, device="cuda")),
                   dict(cloud_of_frame=zeros(3)), dict(xyz=xyz.expand(3, -1, -1), rgb=rgb.expand(3, -1, -1)),
                   dict(background=torch.zeros((2, H, W, 4), dtype=torch.uint8, device="cuda")), dict(background=(1, 2)),
                   dict(out=torch.zeros((2, H, W, 3), dtype=torch.uint8)), dict(out=torch.zeros((1, H, W, 3), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            geometry.render_scene(**{**ok, **change})
    with pytest.raises(ValueError):
        geometry.render_scene(vs, rgb=rgb, size=(H, W))


def test_c_entry_reports_errors_without_a_launch():
    lib, st = _lib.lib(), _lib.current_stream()
    H, W = sc.SIZES[0]
    vs, (xyz, rgb) = dev(sc.views(1, H, W)), (dev(a) for a in cloud(1, 1500, 2))
    out = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(8 * H * W, dtype=torch.uint8, device="cuda")
    pr = dev(sc.counted(1, H, W))
    names = ["views", "xyz", "rgb", "count", "cof", "P", "N", "point_size", "prims", "axes", "M", "bg", "colour", "frames", "depth", "index", "F", "H",
             "W", "ws", "ws_bytes", "stream"]
    good = [vs.data_ptr(), xyz.data_ptr(), rgb.data_ptr(), None, None, 1, 1500, 1, pr.data_ptr(), 2, 1, None, 0, out.data_ptr(), None, None, 1, H, W,
            ws.data_ptr(), ws.numel(), st]

    def call(**change):
        return lib.skimi_scene_view_render(*[change.get(n, v) for n, v in zip(names, good)])

    for change, word in ((dict(views=None), b"NULL"), (dict(frames=None), b"NULL"), (dict(xyz=None), b"NULL"), (dict(prims=None), b"NULL"),
                         (dict(ws=None), b"NULL"), (dict(point_size=0), b"point_size"), (dict(point_size=5), b"point_size"), (dict(M=1025), b"M ="),
                         (dict(axes=4), b"prim_axes"), (dict(F=0), b"F ="), (dict(H=0), b"frame"), (dict(N=-1), b"N ="), (dict(P=2), b"cloud_of_frame"),
                         (dict(ws_bytes=8 * H * W - 1), b"workspace")):
        assert call(**change) != 0, change
        assert word in lib.skimi_last_error(), (change, lib.skimi_last_error())
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert call() == 0
    want, _, _ = sr.render(vs.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy(), None, None, 1, pr.cpu().numpy(), H, W, 0)
    assert (out.cpu().numpy() == want).all()
