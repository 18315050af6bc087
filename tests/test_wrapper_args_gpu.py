"""GPU: what the wrappers behind geometry.<name> do to their tensor arguments before the launch, one valid call per
wrapper at the smallest shape its entry point takes.

Every call is made three times: with contiguous tensors of the wrapper's own float width, with the same values behind
a non-contiguous view (every other column of a buffer twice as wide), and in the other float width (every value is
representable in float32, so widening and narrowing are exact).  The kernels then see the same bits, so the outputs
must be bit-equal (NaN-aware): a wrapper that forgets .contiguous() or converts to the wrong dtype reads garbage and
fails here.  The second half holds the refusals that need device tensors, with the exception class of each.

Only public names are used: the tables describe the wrappers as they were before geometry.py was split as well."""
import dataclasses

import numpy as np
import pytest
import torch

from skiing_analysis_pytorch_amd import _lib, geometry

SkimiError = _lib.SkimiError
FLOATS = (torch.float32, torch.float64)


def dev(a, dtype=None):
    """a host array whose values are float32 numbers -> device tensor of `dtype` (default: the array's own)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def f32_values(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def strided(t):
    """the same values behind a non-contiguous view: every other column of a buffer twice as wide"""
    buf = torch.zeros((*t.shape[:-1], 2 * t.shape[-1]), dtype=t.dtype, device=t.device)
    view = buf[..., ::2]
    view.copy_(t)
    assert not view.is_contiguous() or t.shape[-1] <= 1
    return view


def other_width(t):
    return t.to(torch.float64 if t.dtype == torch.float32 else torch.float32)


def three_ways(args):
    """the tensor arguments of a call: as they are, strided, in the other float width (non-float tensors stay)"""
    is_f = lambda v: isinstance(v, torch.Tensor) and v.dtype in FLOATS      # noqa: E731
    yield "contiguous", args
    yield "strided", {k: strided(v) if is_f(v) else v for k, v in args.items()}
    yield "other width", {k: other_width(v) if is_f(v) else v for k, v in args.items()}


def leaves(r):
    if isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, np.ndarray):
        return [torch.from_numpy(r)]
    if r is None or isinstance(r, str):
        return []
    if isinstance(r, (int, float)):
        return [torch.tensor(float(r), dtype=torch.float64)]
    if dataclasses.is_dataclass(r):
        r = [getattr(r, f.name) for f in dataclasses.fields(r)]
    return [x for item in r for x in leaves(item)]


def assert_bit_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype, a.shape, b.shape)
        if a.dtype.is_floating_point:
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (what, i)
            a, b = torch.nan_to_num(a), torch.nan_to_num(b)
        assert torch.equal(a, b), (what, i)


# ---- a two-camera rig of float32 numbers, built once on the host ---------------------------------------------------
def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _rig():
    rng = np.random.default_rng(7)
    K = f32_values(np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]))
    R = f32_values(np.stack([np.eye(3), _rot_y(0.3)]))
    t = f32_values(np.array([[0.0, 0, 0], [-1.0, 0.05, 0.2]]))
    X = f32_values(rng.uniform(-1, 1, (2, 17, 3)) * [0.5, 0.8, 0.3] + [0, 0, 4.0])          # [T, J, 3]
    cam = np.einsum("vij,tnj->tvni", R, X) + t[None, :, None]
    x2d = f32_values(np.einsum("ij,tvnj->tvni", K, cam / cam[..., 2:])[..., :2] + rng.normal(0, 0.3, (2, 2, 17, 2)))
    conf = f32_values(rng.uniform(0.5, 1.0, (2, 2, 17)))
    return dict(K=K, R=R, t=t, X=X, x2d=x2d, conf=conf, rng=rng)


RIG = _rig()
KV = np.stack([RIG["K"], RIG["K"]])                        # [V, 3, 3]
DIST = f32_values([-0.2, 0.05, 0.001, -0.002, 0.01])
H36M_IDX = dict(root_idx=0, left_hip_idx=4, right_hip_idx=1, left_shoulder_idx=11, right_shoulder_idx=14)


def _steps(dtype=torch.float32):
    """K, R [1, V, 3, 3], t [1, V, 3], keypoints [1, V, J, 2], conf [1, V, J]: T = 1, V = 2, J = 17"""
    return dict(K=dev(KV[None], dtype), R=dev(RIG["R"][None], dtype), t=dev(RIG["t"][None], dtype),
                keypoints=dev(RIG["x2d"][:1], dtype))


def _group8():
    """one group of 8 points seen by V = 2 views"""
    return dict(X=dev(RIG["X"][0, :8]), x2d=dev(RIG["x2d"][0, :, :8]), K=dev(KV), conf=dev(RIG["conf"][0, :, :8]))


def _clip(T, J, seed):
    rng = np.random.default_rng(seed)
    return f32_values(np.cumsum(rng.normal(0, 0.02, (T, J, 3)), axis=0) + rng.uniform(-0.5, 0.5, (1, J, 3)))


def _cloud64():
    rng = np.random.default_rng(3)
    xy = rng.uniform(-0.5, 0.5, (64, 2))
    src = f32_values(np.c_[xy, 0.2 * xy[:, 0] ** 2 - 0.1 * xy[:, 1] + 2.0])
    return src, f32_values(src + [0.01, -0.005, 0.02])


def _board():
    """3 views of a 9 x 6 board: obj [54, 2], img [3, 54, 2]"""
    obj = np.stack(np.meshgrid(np.arange(9.0), np.arange(6.0)), -1).reshape(-1, 2) * 0.025
    img = []
    for ax, ay, tz in ((0.3, -0.2, 0.5), (-0.25, 0.3, 0.6), (0.1, 0.35, 0.45)):
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        cam = np.c_[obj - [0.1, 0.0625], np.zeros(54)] @ (_rot_y(ay) @ Rx).T + [0.01, -0.02, tz]
        img.append((RIG["K"] @ (cam / cam[:, 2:]).T).T[:, :2])
    return f32_values(obj), f32_values(np.stack(img))


def _scene_trim(r):
    """rows at and beyond count are unwritten"""
    n = int(r.count[0])
    return (r.xyz[:, :n], r.rgb[:, :n]) + tuple(r[2:])


def _cases():
    g = geometry
    src, tgt = _cloud64()
    obj, img = _board()
    clip17, clip17b, clip15 = _clip(4, 17, 1), _clip(4, 17, 2), _clip(4, 15, 3)
    rng = np.random.default_rng(11)
    pts5 = f32_values(rng.uniform(100, 500, (5, 2)))
    quad = f32_values([[0, 1080], [1920, 1080], [1336, 130], [600, 130]])
    quad_m = f32_values([[-15, 0], [15, 0], [15, 60], [-15, 60]])
    E1 = f32_values(np.c_[_rot_y(0.1), [0.1, 0.2, 0.3]])
    norm = lambda v: np.linalg.solve(RIG["K"], np.c_[RIG["x2d"][0, v, :5], np.ones(5)].T).T[:, :2]      # noqa: E731
    return {
        "pose_encoding_to_extri_intri": (lambda pe: g.pose_encoding_to_extri_intri(pe, (14, 14)),
                                         dict(pe=dev(f32_values(rng.uniform(-0.5, 0.5, (1, 2, 9))), torch.float32))),
        "unproject_depth_map_to_point_map": (g.unproject_depth_map_to_point_map,
                                             dict(depth=dev(f32_values(rng.uniform(1, 3, (2, 4, 4, 1))), torch.float32),
                                                  extrinsic=dev(np.stack([E1, E1]), torch.float32), intrinsic=dev(KV, torch.float32))),
        "triangulate_joints": (g.triangulate_joints, _steps()),
        "triangulate_triage": (g.triangulate_triage, dict(_steps(), conf=dev(RIG["conf"][:1], torch.float32))),
        "triangulate_triage_dist": (lambda **kw: g.triangulate_triage(dist=DIST, **kw), _steps()),
        "triangulate_robust": (g.triangulate_robust, dict(_steps(), conf=dev(RIG["conf"][:1], torch.float32))),
        "person_origin": (lambda point_maps, boxes: g.person_origin(point_maps, boxes, (4, 4)),
                          dict(point_maps=dev(f32_values(rng.uniform(1, 3, (1, 4, 4, 3))), torch.float32),
                               boxes=dev(f32_values([[0, 0, 4, 4]]), torch.float32))),
        "recenter_cameras": (g.recenter_cameras, dict(stats=dev(f32_values(rng.uniform(1, 9, (1, 2, 8)))),
                                                      extrinsic=dev(np.stack([E1, E1])[None], torch.float32))),
        "scene_point_cloud": (lambda **kw: _scene_trim(g.scene_point_cloud(**kw)),
                              dict(points=dev(f32_values(rng.uniform(-1, 1, (1, 1, 4, 4, 3))), torch.float32),
                                   conf=dev(f32_values(rng.uniform(1, 9, (1, 1, 4, 4))), torch.float32),
                                   images=dev(f32_values(rng.uniform(0, 1, (1, 1, 3, 4, 4))), torch.float32),
                                   extrinsic=dev(E1[None, None], torch.float32))),
        "estimate_normals": (lambda points: g.estimate_normals(points, radius=0.5), dict(points=dev(tgt, torch.float32))),
        "icp_correspondences": (lambda source, target: g.icp_correspondences(source, target, max_distance=0.5),
                                dict(source=dev(src, torch.float32), target=dev(tgt, torch.float32))),
        "icp_point_to_plane": (lambda source, target: g.icp_point_to_plane(source, target, 0.5, 0.5, max_iteration=5),
                               dict(source=dev(src, torch.float32), target=dev(tgt, torch.float32))),
        "bundle_adjust": (lambda **kw: g.bundle_adjust(modes=("pose_only", "full"), num_iters=2, **kw),
                          dict(K=dev(KV), R=dev(np.stack([RIG["R"]] * 2)), t=dev(np.stack([RIG["t"]] * 2)), X=dev(RIG["X"]),
                               x2d=dev(RIG["x2d"]), conf=dev(RIG["conf"]))),
        "relative_pose": (g.relative_pose, dict(R=dev(RIG["R"][None]), t=dev(RIG["t"][None]))),
        "resect_cameras": (g.resect_cameras, _group8()),
        "refine_cameras_points": (lambda **kw: g.refine_cameras_points(lambda_x=1.0, max_evals=5, **kw), _group8()),
        "essential_ransac": (lambda **kw: g.essential_ransac(hypotheses=16, **kw), dict(x2d=dev(RIG["x2d"][0, :, :8]), K=dev(KV))),
        "five_point": (g.five_point, dict(a=dev(f32_values(norm(0))[None]), b=dev(f32_values(norm(1))[None]))),
        "fuse_h36m": (g.fuse_h36m, dict(left_3d=dev(clip17[:2]), right_3d=dev(clip17b[:2]))),
        "fuse_views": (lambda **kw: g.fuse_views(**kw, **H36M_IDX),
                       dict(X_l=dev(RIG["X"]), X_r=dev(f32_values(RIG["X"] @ _rot_y(0.3).T)), U_l=dev(RIG["x2d"][:, 0]),
                            U_r=dev(RIG["x2d"][:, 1]))),
        "smooth_ema": (g.smooth_ema, dict(X=dev(clip17))),
        "smooth_savgol": (g.smooth_savgol, dict(X=dev(clip17))),
        "kinematics": (g.kinematics, dict(X=dev(clip15))),
        "pose_errors": (lambda **kw: g.pose_errors(aligned=True, **kw), dict(pred=dev(clip17), target=dev(clip17b))),
        "clip_quality": (g.clip_quality, dict(X=dev(clip17))),
        "distort_points": (lambda x: g.distort_points(x, RIG["K"], DIST), dict(x=dev(pts5))),
        "undistort_points": (lambda x: g.undistort_points(x, RIG["K"], DIST), dict(x=dev(pts5))),
        "undistort_keypoints_steps": (lambda keypoints, K: g.undistort_keypoints_steps(keypoints, K, DIST),
                                      dict(keypoints=dev(RIG["x2d"][:1]), K=dev(KV[None]))),
        "project_points": (lambda X: g.project_points(X, RIG["R"][1], RIG["t"][1], RIG["K"], DIST), dict(X=dev(RIG["X"][0, :5]))),
        "homography_fit": (g.homography_fit, dict(src=dev(quad), dst=dev(quad_m))),
        "homography_points": (g.homography_points, dict(x=dev(quad), H=dev(f32_values([[0.02, 0.001, -15], [0, -0.06, 64], [0, 1e-4, 1]])))),
        "bev_skeleton": (g.bev_skeleton, dict(X=dev(RIG["X"]), center_px=dev(f32_values([[400, 300], [402, 299]])))),
        "ground_track": (g.ground_track, dict(p=dev(clip17[:, 0, :2]))),
        "calibrate_camera": (lambda obj, img: g.calibrate_camera(obj, img, (640, 480), max_evals=20), dict(obj=dev(obj), img=dev(img))),
    }


@pytest.fixture(scope="module")
def cases():
    return _cases()


CASE_NAMES = ["pose_encoding_to_extri_intri", "unproject_depth_map_to_point_map", "triangulate_joints", "triangulate_triage",
              "triangulate_triage_dist", "triangulate_robust", "person_origin", "recenter_cameras", "scene_point_cloud",
              "estimate_normals", "icp_correspondences", "icp_point_to_plane", "bundle_adjust", "relative_pose", "resect_cameras",
              "refine_cameras_points", "essential_ransac", "five_point", "fuse_h36m", "fuse_views", "smooth_ema", "smooth_savgol",
              "kinematics", "pose_errors", "clip_quality", "distort_points", "undistort_points", "undistort_keypoints_steps",
              "project_points", "homography_fit", "homography_points", "bev_skeleton", "ground_track", "calibrate_camera"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_same_bits_contiguous_strided_and_other_float_width(cases, name):
    assert sorted(cases) == sorted(CASE_NAMES)
    fn, args = cases[name]
    results = {how: [x.cpu() for x in leaves(fn(**a))] for how, a in three_ways(args)}
    want = results["contiguous"]
    floats = [x for x in want if x.dtype.is_floating_point]      # icp_correspondences gives indices alone: some must be found
    assert any(torch.isfinite(x).any() for x in floats) if floats else any((x >= 0).any() for x in want), f"{name}: an empty result"
    for how in ("strided", "other width"):
        assert_bit_equal(results[how], want, f"{name}: {how}")


@pytest.mark.gpu
def test_the_launch_fast_paths_refuse_what_they_would_have_to_convert():
    a = dict(_steps(), conf=dev(RIG["conf"][:1], torch.float32))
    launches = ((geometry.triage_launch, (0.3, 2.0)), (geometry.robust_launch, (0.3, 2.0, 2, 5, False)))
    for launch, tail in launches:
        assert len(launch(a["K"], a["R"], a["t"], a["keypoints"], a["conf"], *tail)) in (7, 8)
        for key in ("K", "keypoints", "conf"):
            for bad in (strided(a[key]), other_width(a[key])):
                b = dict(a, **{key: bad})
                with pytest.raises(ValueError, match=f"{key} must be contiguous float32"):
                    launch(b["K"], b["R"], b["t"], b["keypoints"], b["conf"], *tail)


# ---- refusals before the launch, on device tensors: (call, exception class) ---------------------------------------------
def _refusals():
    g = geometry
    zf = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")      # noqa: E731
    zd = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")      # noqa: E731
    st = lambda **kw: dict(dict(K=zf(1, 2, 3, 3), R=zf(1, 2, 3, 3), t=zf(1, 2, 3), keypoints=zf(1, 2, 17, 2)), **kw)      # noqa: E731
    g8 = lambda **kw: dict(dict(X=zd(8, 3), x2d=zd(2, 8, 2)), **kw)      # noqa: E731
    K3 = RIG["K"]
    return {
        "triage: keypoints' last axis": (lambda: g.triangulate_triage(**st(keypoints=zf(1, 2, 17, 3))), ValueError),
        "triage: K of another shape": (lambda: g.triangulate_triage(**st(K=zf(1, 3, 3, 3))), ValueError),
        "robust: keypoints' last axis": (lambda: g.triangulate_robust(**st(keypoints=zf(1, 2, 17, 3))), ValueError),
        "robust: conf of another shape": (lambda: g.triangulate_robust(**st(conf=zf(1, 2, 16))), ValueError),
        "robust: min_inliers": (lambda: g.triangulate_robust(**st(), min_inliers=1), ValueError),
        "robust: refine_iters": (lambda: g.triangulate_robust(**st(), refine_iters=33), ValueError),
        "robust: inlier_px": (lambda: g.triangulate_robust(**st(), inlier_px=-1.0), ValueError),
        "person_origin: last axis": (lambda: g.person_origin(zf(1, 4, 4, 2), zf(1, 4), (4, 4)), SkimiError),
        "person_origin: boxes": (lambda: g.person_origin(zf(1, 4, 4, 3), zf(2, 4), (4, 4)), SkimiError),
        "recenter: stats": (lambda: g.recenter_cameras(zd(1, 2, 7), zf(1, 2, 3, 4)), ValueError),
        "recenter: extrinsic": (lambda: g.recenter_cameras(zd(1, 2, 8), zf(1, 2, 3, 3)), ValueError),
        "scene: points' last axis": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 2), zf(1, 1, 4, 4), zf(1, 1, 3, 4, 4), zf(1, 1, 3, 4)), ValueError),
        "scene: conf": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 3), zf(1, 1, 4, 5), zf(1, 1, 3, 4, 4), zf(1, 1, 3, 4)), ValueError),
        "scene: images": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 3), zf(1, 1, 4, 4), zf(1, 1, 3, 4, 5), zf(1, 1, 3, 4)), ValueError),
        "scene: extrinsic": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 3), zf(1, 1, 4, 4), zf(1, 1, 3, 4, 4), zf(1, 1, 4, 4)), ValueError),
        "scene: conf_thres": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 3), zf(1, 1, 4, 4), zf(1, 1, 3, 4, 4), zf(1, 1, 3, 4), conf_thres=101), ValueError),
        "scene: capacity": (lambda: g.scene_point_cloud(zf(1, 1, 4, 4, 3), zf(1, 1, 4, 4), zf(1, 1, 3, 4, 4), zf(1, 1, 3, 4), capacity=0), ValueError),
        "normals: last axis": (lambda: g.estimate_normals(zf(64, 2)), SkimiError),
        "icp: last axis": (lambda: g.icp_point_to_plane(zf(64, 3), zf(64, 2)), SkimiError),
        "ba: X's last axis": (lambda: g.bundle_adjust(zd(2, 3, 3), zd(2, 2, 3, 3), zd(2, 2, 3), zd(2, 17, 2), zd(2, 2, 17, 2), zd(2, 2, 17)), ValueError),
        "ba: conf": (lambda: g.bundle_adjust(zd(2, 3, 3), zd(2, 2, 3, 3), zd(2, 2, 3), zd(2, 17, 3), zd(2, 2, 17, 2), zd(2, 2, 16)), ValueError),
        "ba: mode": (lambda: g.bundle_adjust(zd(2, 3, 3), zd(2, 2, 3, 3), zd(2, 2, 3), zd(2, 17, 3), zd(2, 2, 17, 2), zd(2, 2, 17), modes=("nope",)), ValueError),
        "ba: placement": (lambda: g.bundle_adjust(zd(2, 3, 3), zd(2, 2, 3, 3), zd(2, 2, 3), zd(2, 17, 3), zd(2, 2, 17, 2), zd(2, 2, 17), placement="hbm"), ValueError),
        "relative_pose: R": (lambda: g.relative_pose(zd(1, 2, 3, 2), zd(1, 2, 3)), ValueError),
        "relative_pose: t": (lambda: g.relative_pose(zd(1, 2, 3, 3), zd(1, 3, 3)), ValueError),
        "resect: X's last axis": (lambda: g.resect_cameras(**g8(X=zd(8, 2))), ValueError),
        "resect: conf": (lambda: g.resect_cameras(**g8(conf=zd(2, 7))), ValueError),
        "resect: K": (lambda: g.resect_cameras(**g8(K=zd(3, 3, 3))), ValueError),
        "resect: R0 without t0": (lambda: g.resect_cameras(**g8(R0=zd(1, 2, 3, 3))), ValueError),
        "resect: loss": (lambda: g.resect_cameras(**g8(), loss="huber"), ValueError),
        "resect: group_size": (lambda: g.resect_cameras(**g8(), group_size=3), SkimiError),
        "refine: x2d's last axis": (lambda: g.refine_cameras_points(**g8(x2d=zd(2, 8, 3))), ValueError),
        "refine: t0": (lambda: g.refine_cameras_points(**g8(R0=zd(1, 2, 3, 3), t0=zd(1, 2, 2))), ValueError),
        "refine: loss": (lambda: g.refine_cameras_points(**g8(), loss="huber"), ValueError),
        "refine: group_size": (lambda: g.refine_cameras_points(**g8(), group_size=3), SkimiError),
        "essential: x2d's last axis": (lambda: g.essential_ransac(zd(2, 8, 3), zd(2, 3, 3)), ValueError),
        "essential: K": (lambda: g.essential_ransac(zd(2, 8, 2), zd(3, 3, 3)), ValueError),
        "essential: conf": (lambda: g.essential_ransac(zd(2, 8, 2), zd(2, 3, 3), conf=zd(2, 7)), ValueError),
        "five_point: last axis": (lambda: g.five_point(zd(1, 5, 3), zd(1, 5, 3)), ValueError),
        "five_point: b": (lambda: g.five_point(zd(1, 5, 2), zd(2, 5, 2)), ValueError),
        "fuse_h36m: last axis": (lambda: g.fuse_h36m(zd(2, 17, 2), zd(2, 17, 2)), ValueError),
        "fuse_h36m: right": (lambda: g.fuse_h36m(zd(2, 17, 3), zd(3, 17, 3)), ValueError),
        "fuse_h36m: tau": (lambda: g.fuse_h36m(zd(2, 17, 3), zd(2, 17, 3), tau=np.zeros(16)), ValueError),
        "fuse_h36m: wL": (lambda: g.fuse_h36m(zd(2, 17, 3), zd(2, 17, 3), wL=zd(3)), ValueError),
        "fuse_views: last axis": (lambda: g.fuse_views(zd(2, 17, 2), zd(2, 17, 2), zd(2, 17, 2), zd(2, 17, 2), **H36M_IDX), ValueError),
        "fuse_views: U_r": (lambda: g.fuse_views(zd(2, 17, 3), zd(2, 17, 3), zd(2, 17, 2), zd(2, 16, 2), **H36M_IDX), ValueError),
        "fuse_views: scale_mode": (lambda: g.fuse_views(zd(2, 17, 3), zd(2, 17, 3), zd(2, 17, 2), zd(2, 17, 2), scale_mode="arm", **H36M_IDX), ValueError),
        "smooth_ema: last axis": (lambda: g.smooth_ema(zd(4, 17, 2)), ValueError),
        "smooth_ema: target_ids": (lambda: g.smooth_ema(zd(4, 17, 3), target_ids=range(16)), ValueError),
        "smooth_savgol: last axis": (lambda: g.smooth_savgol(zd(4, 17, 2)), ValueError),
        "smooth_savgol: poly": (lambda: g.smooth_savgol(zd(12, 17, 3), win=5, poly=5), SkimiError),
        "kinematics: last axis": (lambda: g.kinematics(zd(4, 15, 2)), ValueError),
        "kinematics: lengths": (lambda: g.kinematics(zd(4, 15, 3), lengths=[4, 4]), ValueError),
        "kinematics: layout": (lambda: g.kinematics(zd(4, 15, 3), layout=range(12)), ValueError),
        "kinematics: placement": (lambda: g.kinematics(zd(4, 15, 3), placement="lds"), ValueError),
        "pose_errors: last axis": (lambda: g.pose_errors(zd(4, 17, 2), zd(4, 17, 2)), ValueError),
        "pose_errors: target": (lambda: g.pose_errors(zd(4, 17, 3), zd(4, 16, 3)), ValueError),
        "pose_errors: lengths": (lambda: g.pose_errors(zd(4, 17, 3), zd(4, 17, 3), lengths=[4, 4]), ValueError),
        "clip_quality: last axis": (lambda: g.clip_quality(zd(4, 17, 2)), ValueError),
        "clip_quality: lengths": (lambda: g.clip_quality(zd(4, 17, 3), lengths=[]), ValueError),
        "clip_quality: edges": (lambda: g.clip_quality(zd(4, 17, 3), edges=[(0, 1)] * 129), ValueError),
        "clip_quality: placement": (lambda: g.clip_quality(zd(4, 17, 3), placement="lds"), ValueError),
        "distort: last axis": (lambda: g.distort_points(zd(5, 3), K3, DIST), ValueError),
        "distort: dist": (lambda: g.distort_points(zd(5, 2), K3, np.zeros(3)), ValueError),
        "undistort: iters": (lambda: g.undistort_points(zd(5, 2), K3, DIST, iters=1001), ValueError),
        "undistort: cameras": (lambda: g.undistort_points(zd(9, 5, 2), np.stack([K3] * 9), DIST), ValueError),
        "undistort: points per camera": (lambda: g.undistort_points(zd(3, 5, 2), np.stack([K3] * 2), DIST), ValueError),
        "undistort: P": (lambda: g.undistort_points(zd(2, 5, 2), np.stack([K3] * 2), DIST, P=np.stack([K3] * 3)), ValueError),
        "project: last axis": (lambda: g.project_points(zd(5, 2), np.eye(3), np.zeros(3), K3), ValueError),
        "project: t": (lambda: g.project_points(zd(5, 3), np.eye(3), np.zeros(2), K3), ValueError),
        "keypoints_steps: last axis": (lambda: g.undistort_keypoints_steps(zd(1, 2, 17, 3), zd(1, 2, 3, 3), DIST), ValueError),
        "keypoints_steps: K": (lambda: g.undistort_keypoints_steps(zd(1, 2, 17, 2), zd(1, 3, 3, 3), DIST), ValueError),
        "keypoints_steps: dist": (lambda: g.undistort_keypoints_steps(zd(1, 2, 17, 2), zd(1, 2, 3, 3), np.zeros((3, 5))), ValueError),
        "homography_fit: last axis": (lambda: g.homography_fit(zd(4, 3), zd(4, 3)), ValueError),
        "homography_fit: dst": (lambda: g.homography_fit(zd(4, 2), zd(5, 2)), ValueError),
        "homography_fit: n": (lambda: g.homography_fit(zd(3, 2), zd(3, 2)), ValueError),
        "homography_fit: post": (lambda: g.homography_fit(zd(4, 2), zd(4, 2), post=np.eye(2)), ValueError),
        "homography_points: last axis": (lambda: g.homography_points(zd(4, 3), zd(3, 3)), ValueError),
        "homography_points: H": (lambda: g.homography_points(zd(2, 4, 2), zd(3, 3, 3)), ValueError),
        "homography_points: eps": (lambda: g.homography_points(zd(4, 2), zd(3, 3), eps=-1.0), ValueError),
        "bev_skeleton: last axis": (lambda: g.bev_skeleton(zd(2, 17, 2), zd(2, 2)), ValueError),
        "bev_skeleton: center_px": (lambda: g.bev_skeleton(zd(2, 17, 3), zd(3, 2)), ValueError),
        "bev_skeleton: center_world": (lambda: g.bev_skeleton(zd(2, 17, 3), zd(2, 2), center_world=zd(2, 2)), ValueError),
        "bev_skeleton: use_axes": (lambda: g.bev_skeleton(zd(2, 17, 3), zd(2, 2), use_axes=(0, 3)), ValueError),
        "bev_skeleton: metres_per_pixel": (lambda: g.bev_skeleton(zd(2, 17, 3), zd(2, 2), metres_per_pixel=0.0), ValueError),
        "ground_track: last axis": (lambda: g.ground_track(zd(4, 3)), ValueError),
        "ground_track: fps": (lambda: g.ground_track(zd(4, 2), fps=0.0), ValueError),
        "calibrate: obj's last axis": (lambda: g.calibrate_camera(zd(54, 3), zd(3, 54, 2), (640, 480)), ValueError),
        "calibrate: img": (lambda: g.calibrate_camera(zd(54, 2), zd(3, 53, 2), (640, 480)), ValueError),
        "calibrate: use": (lambda: g.calibrate_camera(zd(54, 2), zd(3, 54, 2), (640, 480), use=torch.ones(1, 2, dtype=torch.bool, device="cuda")), ValueError),
        "calibrate: K0 against dist0": (lambda: g.calibrate_camera(zd(54, 2), zd(3, 54, 2), (640, 480), K0=zd(2, 3, 3), dist0=zd(3, 5)), ValueError),
        "calibrate: dist0": (lambda: g.calibrate_camera(zd(54, 2), zd(3, 54, 2), (640, 480), dist0=zd(13)), ValueError),
        "calibrate: free": (lambda: g.calibrate_camera(zd(54, 2), zd(3, 54, 2), (640, 480), free=("fx", "zz")), ValueError),
    }


@pytest.mark.gpu
def test_refusals_before_the_launch_keep_their_exception_class():
    table = _refusals()
    for what, (call, exc) in table.items():
        with pytest.raises(exc) as e:
            call()
        assert type(e.value) is exc, (what, type(e.value))      # SkimiError is no ValueError and the reverse
        print(f"{what}: {exc.__name__}: {e.value}")
