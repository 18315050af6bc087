"""CPU: the rules of the scene-view renderer.  The NumPy restatement (tests/scene_view_restated.py) against a brute-force
painter written differently, the depth formulas, the near-plane clip, the orbit views, the torch builders against their NumPy
restatement, and the identity case.  No GPU: the device is compared with the restatement in tests/test_scene_view_gpu.py."""
import math

import numpy as np
import pytest
import torch

import scene_view_cases as sc
import scene_view_restated as sr
from skiing_analysis_pytorch_amd import geometry


def _cases():
    """name -> (views, xyz, rgb, count, cloud_of_frame, point_size, prims, H, W, background)"""
    (H0, W0), (H1, W1) = sc.SIZES
    xyz, rgb = sc.cloud(1)
    xyz2, rgb2 = sc.cloud(2, N=700, seed=4)
    out = {
        "persp_cloud_prims": (sc.views(1, H0, W0), xyz, rgb, None, None, 1, sc.random_prims(64, H0, W0, 1), H0, W0, 0),
        "ortho_size3_special": (sc.views(1, H0, W0, True), xyz, rgb, np.array([3000]), None, 3, sc.special_prims(H0, W0), H0, W0, (9, 8, 7)),
        "two_clouds_per_frame_lists": (sc.views(2, H1, W1), xyz2, rgb2, np.array([700, 350]), np.array([1, 0]), 2,
                                       np.stack([sc.random_prims(20, H1, W1, 2), sc.random_prims(20, H1, W1, 3)]), H1, W1, 255),
        "one_tile_300": (sc.views(1, H0, W0), None, None, None, None, 1, sc.one_tile(300), H0, W0, 0),
        "cloud_only_size4": (sc.views(1, H0, W0), xyz, rgb, None, None, 4, None, H0, W0, 0),
    }
    for ortho in (False, True):
        v, x, c, p, _ = sc.plane_case(H0, W0, ortho)
        out[f"plane_{'ortho' if ortho else 'persp'}"] = (v, x, c, None, None, 1, p, H0, W0, 0)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_brute_force_painter(name):
    args = CASES[name]
    f1, d1, i1 = sr.render(*args)
    f2, d2, i2 = sr.paint_brute(*args)
    assert (f1 == f2).all() and (i1 == i2).all()
    assert (d1.view(np.uint32) == d2.view(np.uint32)).all()
    bg = sr.background_frames(args[-1], len(args[0]), args[-3], args[-2])
    assert (f1 != bg).any(), "the case draws nothing"


def test_cloud_case_is_what_it_claims():
    H, W = sc.SIZES[0]
    xyz, _ = sc.cloud(1)
    for ortho in (False, True):
        view = sc.views(1, H, W, ortho)[0]
        ok, u, v, q = sr.project(view, xyz[0])
        with np.errstate(all="ignore"):
            fu, fv = np.floor(u), np.floor(v)
        assert (~ok).sum() >= 30                                                      # non-finite, behind near, beyond far
        assert (ok & (fu < 0)).any() and (ok & (fu >= W)).any() and (ok & (fv < 0)).any() and (ok & (fv >= H)).any()
        inside = ok & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        pix = (fv[inside] * W + fu[inside]).astype(np.int64)
        assert len(pix) - len(np.unique(pix)) >= 300                                  # several hundred share pixels
        key = pix * (1 << 31) + q[inside].astype(np.int64)
        assert len(key) - len(np.unique(key)) >= 24                                   # dozens share a pixel AND w
        # squares of size 3 are cut by each edge
        assert (inside & (fu == 0)).any() and (inside & (fu == W - 1)).any() and (inside & (fv == 0)).any() and (inside & (fv == H - 1)).any()


def test_plane_case_has_the_capsule_on_both_sides():
    for ortho in (False, True):
        v, x, c, p, wp = sc.plane_case(*sc.SIZES[0], ortho)
        H, W = sc.SIZES[0]
        frames, depth, index = sr.render(v, x, c, None, None, 1, p, H, W)
        wm = sr.fragment_map(p[0], H, W)
        pt = index[0] >= 0
        assert ((wm > wp) & pt).any() and ((wm > 0) & (wm < wp) & pt).any()
        cap = np.array([255, 0, 255], dtype=np.uint8)
        assert (frames[0][(wm > wp) & pt] == cap).all() and not (frames[0][(wm > 0) & (wm < wp) & pt] == cap).all(axis=-1).any()
        # the disc of the plane's own w covers its points, the one a step behind does not
        d0, d1 = sr.fragment_map(p[1], H, W) > 0, sr.fragment_map(p[2], H, W) > 0
        assert (frames[0][d0 & pt & (wm <= wp)] == [0, 255, 0]).all() and (d0 & pt).any()
        only1 = d1 & ~d0 & pt & (wm < wp)
        assert only1.any() and not (frames[0][only1] == [255, 0, 0]).all(axis=-1).any()


def test_depth_is_monotone_and_decodes():
    Z = np.linspace(sc.NEAR, sc.FAR, 4001)
    pts = np.stack([Z, np.zeros_like(Z), np.zeros_like(Z)], axis=1).astype(np.float32)
    for ortho in (False, True):
        view = sr.look_at([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], 10.0, 10.0, 5.0, 5.0, sc.NEAR, sc.FAR, ortho)
        ok, _, _, q = sr.project(view, pts)
        assert ok[1:-1].all() and (np.diff(q[ok]) <= 0).all() and q[ok].max() <= sr.W_ONE and q[ok].min() >= 1
        assert len(np.unique(q[ok])) == ok.sum()                   # 4001 depths, 4001 different w
        back = sr.decode_depth(view, q[ok].astype(np.int64)).astype(np.float64)
        zs = pts[ok, 0].astype(np.float64)
        # floor loses at most one step of w: dZ = Z^2 / (2^30 near) (perspective), (far - near) / 2^30 (orthographic), plus float32
        step = (sc.FAR - sc.NEAR) / sr.W_ONE if ortho else zs * zs / (sr.W_ONE * sc.NEAR)
        assert (back >= zs - 1e-7 * zs).all() and (back - zs <= step + 2.0 ** -23 * zs).all()
    assert sr.decode_depth(view, np.array([0]))[0] == np.inf


def test_near_plane_clip_cross_touch_miss():
    near = 0.5
    segs = {
        "in front": ((0.0, 0.0, 1.0), (1.0, 1.0, 2.0)),
        "crosses, a behind": ((0.0, 0.0, -0.5), (2.0, 4.0, 1.5)),
        "crosses, b behind": ((2.0, 4.0, 1.5), (0.0, 0.0, -0.5)),
        "touches": ((0.0, 0.0, 0.5), (1.0, 0.0, 0.25)),
        "misses": ((0.0, 0.0, 0.1), (1.0, 0.0, 0.49)),
        "both on the plane": ((0.0, 0.0, 0.5), (1.0, 0.0, 0.5)),
    }
    a = torch.tensor([s[0] for s in segs.values()], dtype=torch.float64)
    b = torch.tensor([s[1] for s in segs.values()], dtype=torch.float64)
    Xa, Ya, Za, Xb, Yb, Zb, kept = geometry.clip_near(a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2], torch.tensor(near, dtype=torch.float64))
    assert kept.tolist() == [True, True, True, True, False, True]
    for k, (pa, pb) in enumerate(segs.values()):
        want = sr.clip_segment(pa, pb, near)
        assert (want is not None) == bool(kept[k])
        if want is not None:
            got = np.array([[Xa[k], Ya[k], Za[k]], [Xb[k], Yb[k], Zb[k]]], dtype=np.float64)
            assert np.abs(got - np.stack(want)).max() < 1e-12
    assert Za[1] == near and (Xa[1], Ya[1]) == (1.0, 2.0) and Zb[2] == near and Zb[3] == near and (Xb[3], Yb[3]) == (0.0, 0.0)
    # as records: the missed segment is kind 0, the crossing one ends on the plane with w = 2^30
    view = torch.tensor(sr.look_at([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0], 20.0, 20.0, 30.0, 30.0, near, 10.0))
    rec = geometry.segment3d_prims(a, b, view, (1, 2, 3), 2.0)
    assert rec[:, 0].tolist() == [2, 2, 2, 2, 0, 2] and (rec[4] == 0).all()
    assert rec[1, 7] == sr.W_ONE and rec[2, 8] == sr.W_ONE and rec[0, 7] == sr.W_ONE // 2


def test_orbit_view_matches_hand_computed_eyes():
    c = [0.1, -0.2, 0.9]
    hand = {(0, -90): (0.0, -2.0, 0.0), (0, 90): (0.0, 2.0, 0.0), (0, 0): (2.0, 0.0, 0.0), (90, -90): (0.0, 0.0, 2.0), (90, 90): (0.0, 0.0, 2.0),
            (-90, 0): (0.0, 0.0, -2.0), (30, 60): (2 * math.cos(math.pi / 6) * 0.5, 2 * math.cos(math.pi / 6) * math.sqrt(3) / 2, 1.0)}
    for (el, az), off in hand.items():
        v = geometry.orbit_view(c, 2.0, el, az, 50.0, 50.0, 20.0, 20.0, 0.1, 9.0, ortho=True)
        assert v.shape == (20,) and v.dtype == torch.float64 and torch.isfinite(v).all(), (el, az)
        M = v[:12].reshape(3, 4).numpy()
        R, t = M[:, :3], M[:, 3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert np.abs(-R.T @ t - (np.array(c) + off)).max() < 1e-12
        assert np.abs(R @ np.array(c) + t - [0, 0, 2.0]).max() < 1e-12              # the centre is straight ahead
        assert np.abs(v[12:].numpy() - [50, 50, 20, 20, 0.1, 9.0, 1, 0]).max() == 0
        if abs(el) != 90:
            assert R[1, 2] < 0                                                        # world +z points up the screen
    # matplotlib's top view at (90, -90): x to the right, y up; the restated look_at agrees elsewhere
    R = geometry.orbit_view(c, 2.0, 90, -90, 1, 1, 0, 0, 0.1, 9.0)[:12].reshape(3, 4)[:, :3].numpy()
    assert np.abs(R - [[1, 0, 0], [0, -1, 0], [0, 0, -1]]).max() < 1e-12
    got = geometry.orbit_view(c, 2.0, 30.0, 60.0, 50.0, 40.0, 20.0, 21.0, 0.1, 9.0).numpy()
    want = sr.look_at(sr.orbit_eye(c, 2.0, 30.0, 60.0), c, [0, 0, 1], 50.0, 40.0, 20.0, 21.0, 0.1, 9.0)
    assert np.abs(got - want).max() < 1e-12
    # the top and bottom views at every azimuth: the up vector is -sign(el) (cos az, sin az, 0), the limit of the +z-up frame, so
    # the view turns continuously into the top view as the elevation approaches 90 degrees
    for el in (90.0, -90.0):
        for az in (-90.0, 90.0, 0.0, 37.0):
            top = geometry.orbit_view(c, 2.0, el, az, 1, 1, 0, 0, 0.1, 9.0).numpy()
            near = geometry.orbit_view(c, 2.0, el * (1 - 1e-7), az, 1, 1, 0, 0, 0.1, 9.0).numpy()
            assert np.isfinite(top).all() and np.abs(top - near).max() < 1e-6, (el, az)
            R = top[:12].reshape(3, 4)[:, :3]
            a = math.radians(az)
            assert np.abs(-R[1] - np.array([math.cos(a), math.sin(a), 0.0]) * (-1 if el > 0 else 1)).max() < 1e-12      # screen up
    # batched angles
    vb = geometry.orbit_view(c, 2.0, torch.tensor([0.0, 90.0, 90.0]), torch.tensor([-90.0, -90.0, 90.0]), 1, 1, 0, 0, 0.1, 9.0)
    assert vb.shape == (3, 20) and torch.isfinite(vb).all()


@pytest.mark.parametrize("ortho", [False, True])
def test_torch_builders_agree_with_the_numpy_restatement(ortho):
    H, W = sc.SIZES[1]
    vs = sc.views(3, H, W, ortho)
    rng = np.random.default_rng(9)
    p0, p1 = rng.uniform(-1.5, 1.5, (40, 3)), rng.uniform(-1.5, 1.5, (40, 3))
    p0[:6] = rng.uniform(2.0, 4.0, (6, 1)) * np.array([1.0, 0.0, 0.2])              # behind / around the cameras: the clip works
    p0[7, 1] = np.nan
    colour = 0x0A0B0C
    seg = geometry.segment3d_prims(torch.from_numpy(p0), torch.from_numpy(p1), torch.from_numpy(vs), (12, 11, 10), 2.5).numpy()
    disc = geometry.disc3d_prims(torch.from_numpy(p0), torch.from_numpy(vs), (12, 11, 10), 3.0).numpy()
    xy, w, ok = geometry.view_project(torch.from_numpy(p0), torch.from_numpy(vs))
    assert seg.shape == (3, 40, 12) and seg.dtype == np.int32 and disc.shape == (3, 40, 12)
    assert xy.shape == (3, 40, 2) and w.dtype == torch.int32 and ok.dtype == torch.bool
    kinds = set()
    for f in range(3):
        for k in range(40):
            for got, want in ((seg[f, k], sr.segment_prim(vs[f], p0[k], p1[k], colour, 2.5)), (disc[f, k], sr.disc_prim(vs[f], p0[k], colour, 3.0))):
                # two correctly rounded f64 evaluations in different orders: one grid unit in position, one step in w
                assert got[0] == want[0] and got[5] == want[5] and got[6] == want[6] and (got[9:] == 0).all(), (f, k, got, want)
                assert np.abs(got[1:5].astype(np.int64) - want[1:5]).max() <= 1 and np.abs(got[7:9].astype(np.int64) - want[7:9]).max() <= 1, (f, k, got, want)
                kinds.add(int(got[0]))
            pr = sr.project_camera(vs[f], sr.to_camera(vs[f], p0[k])) if np.isfinite(p0[k]).all() else None
            assert bool(ok[f, k]) == (pr is not None)
            if pr is not None:
                assert abs(float(xy[f, k, 0]) - pr[0]) < 1e-9 and abs(float(xy[f, k, 1]) - pr[1]) < 1e-9 and abs(int(w[f, k]) - pr[2]) <= 1
    assert kinds == {0, 1, 2}
    # view_project is the splat pass's projection, bit for bit
    okr, u, v, q = sr.project(vs[1], p0.astype(np.float32))
    xy32, w32, ok32 = geometry.view_project(torch.from_numpy(p0.astype(np.float32)), torch.from_numpy(vs[1]))
    assert (ok32.numpy() == okr).all() and (xy32.numpy()[okr, 0] == u[okr]).all() and (xy32.numpy()[okr, 1] == v[okr]).all()
    assert (w32.numpy()[okr] == q[okr]).all()


def test_composite_builders_shapes_and_nan_handling():
    H, W = sc.SIZES[1]
    vs = torch.from_numpy(sc.views(2, H, W))
    j = torch.from_numpy(sc.skeleton_clip(2))
    links = [(0, 1), (1, 2), (2, 3), (3, 4), (99, 1)]
    sk = geometry.skeleton_prims(j, links, vs)
    assert sk.shape == (2, 4 + 17, 12) and sk.dtype == torch.int32
    assert sk[0, 2, 0] == 0 and sk[0, 3, 0] == 0 and sk[0, 4 + 3, 0] == 0 and sk[1, 2, 0] == 2 and sk[1, 4 + 3, 0] == 1   # joint 3 of frame 0 is NaN
    E = torch.eye(4, dtype=torch.float64)[None, :3].repeat(3, 1, 1)
    E[:, 2, 3] = torch.tensor([2.0, 2.5, 3.0])
    K = torch.tensor([[100.0, 0, 64], [0, 100.0, 36], [0, 0, 1]], dtype=torch.float64).repeat(3, 1, 1)
    cam = geometry.camera_prims(E, K, vs, axis_len=0.2, frustum_depth=0.3)
    assert cam.shape == (2, 3 * geometry.CAMERA_PRIMS_PER_CAMERA, 12)
    assert cam[0, :3, 6].tolist() == [geometry.pack_colour(c) for c in geometry.CAMERA_AXIS_COLOURS]
    assert np.abs(geometry.camera_centres(E).numpy() - [[0, 0, -2.0], [0, 0, -2.5], [0, 0, -3.0]]).max() == 0
    g = geometry.grid_prims("xy", 0.5, 0.25, vs)
    assert g.shape == (2, 10, 12) and (g[..., 0] == 2).all()
    allp = geometry.cat_prims(g[0], sk, cam)
    assert allp.shape == (2, 10 + 21 + 33, 12) and allp.is_contiguous() and (allp[1, :10] == g[0]).all()
    one = geometry.views_from_cameras(E, K, near=0.1, far=50.0)
    assert one.shape == (3, 20) and (one[:, :12].reshape(3, 3, 4) == E).all() and one[0, 12:].tolist() == [100, 100, 64, 36, 0.1, 50.0, 0, 0]


def test_identity_case_shows_every_point_in_its_own_pixel():
    view, xyz, rgb, (H, W) = sc.identity_case()
    frames, depth, index = sr.render(view, xyz, rgb, None, None, 1, None, H, W, background=0)
    assert (index[0].reshape(-1) == np.arange(H * W)).all()
    assert (frames[0].reshape(-1, 3) == rgb[0]).all()
    assert np.isfinite(depth).all() and depth.min() >= 1.0 - 1e-6 and depth.max() <= 3.0 + 1e-6
