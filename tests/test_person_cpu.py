"""CPU: the float64 restatement of the person origin and the triage (tests/person_restated.py) against what this
repository already has and against the reference's formulas, fuse.smooth_skeleton against scipy, and the argument
checks of the new entry points (no GPU: nothing is launched).

Seven of these tests validate the restatement itself (against extract_person_points, recenter_and_align, NumPy, the
reference's formulas and its recorded post_triage_sequence) and use nothing else that is new: they fail on the parent
commit only because tests/person_restated.py does not exist there.  The tests of fuse.smooth_skeleton, of the argument
checks and of the GPU cases' margins need the feature itself."""
import ctypes

import numpy as np
import pytest
import torch

import person_restated as ref
from skiing_analysis_pytorch_amd import _lib, fuse, geometry
from skiing_analysis_pytorch_amd import multi_view_process as mv

SOURCE = (1080, 1920)


def seeded_map(seed, H=518, W=518):
    """person depth 5 +- 0.4, 30 % background at 20 +- 3, 1 % NaN, 0.5 % inf; a random box in the 1080 x 1920 source"""
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, 1.0, (H, W, 3)).astype(np.float32)
    z = rng.normal(5.0, 0.4, (H, W))
    bg = rng.random((H, W)) < 0.30
    z[bg] = rng.normal(20.0, 3.0, int(bg.sum()))
    P[..., 2] = z.astype(np.float32)
    flat = P.reshape(-1)
    flat[rng.random(flat.size) < 0.01] = np.nan
    flat[rng.random(flat.size) < 0.005] = np.inf
    x = np.sort(rng.uniform(0, SOURCE[1], 2))
    y = np.sort(rng.uniform(0, SOURCE[0], 2))
    box = np.array([x[0], y[0], max(x[1], x[0] + 60), max(y[1], y[0] + 60)]).astype(np.float32).astype(np.float64)
    return P, box


def test_restatement_keeps_the_points_extract_person_points_keeps():
    """The float64 rules against this repository's float32 host function on 20 seeded 518 x 518 maps: the kept SETS are
    identical (the same points in the same order).  The origins then differ only by the float32 summation of the old
    function's `.mean(axis=0)`: measured on these 20 seeds (614 248 valid points) the largest difference is 6.13e-5, at
    seed 16 (67 513 kept points, depths up to ~30); the bound is that with a factor 4, and it judges the old float32
    path, not the new code."""
    worst, total = 0.0, 0
    for seed in range(20):
        P, box = seeded_map(seed)
        old = mv.extract_person_points(P, box, SOURCE)
        new = ref.person_origin(P, box, SOURCE)
        c = ref.crop(box, P.shape[:2], SOURCE)
        crop = P[c[1]:c[3], c[0]:c[2]].reshape(-1, 3)
        valid = crop[np.isfinite(crop).all(axis=1)]
        assert new["n_valid"] == len(valid) and new["n_box"] == len(crop)
        assert np.array_equal(old, valid[new["kept"]]), seed
        assert new["n_kept"] == len(old) > 0
        total += len(valid)
        worst = max(worst, float(np.abs(old.mean(axis=0).astype(np.float64) - new["origin"]).max()))
    print(f"kept sets identical over {total} valid points; largest origin difference {worst:.3e}")
    assert worst < 4 * 6.13e-5


def test_restated_median_and_std_are_numpys_in_float64():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 8, 1001):
        P = rng.normal(size=(1, n, 3)).astype(np.float32)
        r = ref.person_origin(P, [0, 0, n, 1], (1, n))
        z = P[0, :, 2].astype(np.float64)
        assert r["n_valid"] == n and r["median"] == np.median(z)
        assert abs(r["std"] - np.std(z)) <= 1e-15 * (1 + np.std(z))
    # std = 0 keeps nothing (strict <), as the reference
    P = np.full((4, 4, 3), 2.5, np.float32)
    r = ref.person_origin(P, [0, 0, 4, 4], (4, 4))
    assert r["std"] == 0 and r["n_kept"] == 0 and np.isnan(r["origin"]).all()


def test_crop_rules():
    assert ref.crop([0, 0, 1920, 1080], (518, 518), SOURCE) == (0, 0, 518, 518)
    assert ref.crop([-500, -500, 5000, 5000], (518, 518), SOURCE) == (0, 0, 518, 518)
    assert ref.crop([100, 100, 50, 300], (518, 518), SOURCE) is None            # inverted
    assert ref.crop([2000, 0, 2100, 1080], (518, 518), SOURCE) == (517, 0, 518, 518)   # to the right: x1 -> W - 1, x2 -> W
    assert ref.crop([-300, 0, -10, 1080], (518, 518), SOURCE) is None           # to the left: x1 -> 0, x2 -> 0
    assert ref.crop([1918, 0, 2100, 1080], (518, 518), SOURCE) == (517, 0, 518, 518)
    assert ref.crop([-0.9, 0.9, 3.9, 3.2], (10, 10), (10, 10)) == (0, 0, 3, 3)  # truncation toward zero, not floor
    assert ref.crop([float("nan"), 0, 5, 5], (10, 10), (10, 10)) is None


def _reference_smooth(X, win=9, poly=2):
    """triangulation/postprocess.py:54-67 with scipy's filter"""
    from scipy.signal import savgol_filter
    Xs = X.copy()
    T, J, C = X.shape
    win = min(win if win % 2 == 1 else win + 1, max(1 if T % 2 == 1 else T - 1, 3))
    for j in range(J):
        for c in range(C):
            vec = X[:, j, c]
            mask = np.isfinite(vec)
            if mask.sum() >= win:
                v = vec.copy()
                v[mask] = savgol_filter(vec[mask], window_length=win, polyorder=poly)
                Xs[:, j, c] = v
    return Xs


@pytest.mark.parametrize("T", [1, 2, 8, 9, 10, 50])
def test_smooth_skeleton_matches_scipy(T):
    pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(T)
    X = np.cumsum(rng.normal(scale=0.1, size=(T, 17, 3)), axis=0) + rng.normal(size=(1, 17, 3))
    got, want = fuse.smooth_skeleton(X), _reference_smooth(X)
    assert got.shape == X.shape and np.abs(got - want).max() <= 1e-12
    if T % 2 == 1 and T >= 3:
        assert np.abs(got - X).max() <= 1e-12      # the reference's window rule: 3 for every odd T, which a parabola interpolates


def test_smooth_skeleton_nan_gaps_and_short_series():
    pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    X = np.cumsum(rng.normal(scale=0.1, size=(40, 5, 3)), axis=0)
    X[3:6, 0] = np.nan                   # a gap: the finite samples are filtered as one series
    X[::2, 1, 1] = np.nan
    X[:35, 2, 0] = np.nan                # 5 finite samples < window 9: left as it is
    X[:, 3] = np.nan
    got, want = fuse.smooth_skeleton(X), _reference_smooth(X)
    assert np.array_equal(np.isnan(got), np.isnan(X))
    assert np.nanmax(np.abs(got - want)) <= 1e-12
    assert np.array_equal(got[35:, 2, 0], X[35:, 2, 0])
    even = fuse.smooth_skeleton(X, win=8)          # an even window is made odd (9)
    assert np.array_equal(even, got, equal_nan=True)


def _two_view_case(seed=0, J=17):
    """consistent observations of J points by two cameras, view 0 at the origin (R = I, t = 0)"""
    rng = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation
    K = np.array([[[600.0, 0, 320], [0, 610, 240], [0, 0, 1]], [[590.0, 0, 330], [0, 600, 235], [0, 0, 1]]])
    R = np.stack([np.eye(3), Rotation.from_rotvec([0.02, -0.35, 0.01]).as_matrix()])
    t = np.array([[0.0, 0, 0], [1.5, 0.05, 0.3]])
    X = rng.normal(size=(J, 3)) * [0.5, 0.8, 0.4] + [0, 0, 6.0]
    kp = np.empty((2, J, 2))
    for v in range(2):
        p = (X @ R[v].T + t[v]) @ K[v].T
        kp[v] = p[:, :2] / p[:, 2:3]
    return K, R, t, kp, X


def test_triage_with_first_camera_at_origin_is_the_references_reprojection():
    """With R_0 = I, t_0 = 0 projecting every view through its own camera is vggt/reproject.py:108-144 (view 0 through
    K [I | 0], view 1 through the relative pose), and post_triage_single's e1, e2, em (postprocess.py:38-43)."""
    K, R, t, kp, X = _two_view_case()
    kp = kp + np.random.default_rng(1).normal(scale=0.8, size=kp.shape)
    r = ref.triage(K[None], R[None], t[None], kp[None], X[None])
    R_rel = R[1] @ R[0].T
    t_rel = t[1] - R_rel @ t[0]
    want = ref.reproject_two_views(K, R_rel, t_rel, kp, X)
    assert np.abs(r["err"][0] - want).max() < 1e-10
    assert np.abs(r["em"][0] - 0.5 * (want[0] + want[1])).max() < 1e-10
    assert np.abs(r["view_stats"][0, :, 0] - np.sqrt((want ** 2).mean(axis=1))).max() < 1e-10
    assert np.abs(r["view_stats"][0, :, 3] - want.max(axis=1)).max() < 1e-10
    # ... and with t_0 != 0 the two differ: the reason each view goes through its own camera
    t2 = t + R @ np.array([0.3, -0.2, 1.0])
    X2 = X - np.array([0.3, -0.2, 1.0])
    own = ref.triage(K[None], R[None], t2[None], kp[None], X2[None])["err"][0]
    assert np.abs(own - want).max() < 1e-9                       # the same scene, moved: the same errors
    R_rel2 = R[1] @ R[0].T
    assert np.abs(ref.reproject_two_views(K, R_rel2, t2[1] - R_rel2 @ t2[0], kp, X2) - want).max() > 1.0


def test_triage_keep_conditions_one_by_one():
    K, R, t, kp, X = _two_view_case(seed=2, J=6)
    conf = np.full((2, 6), 0.9)
    base = ref.triage(K[None], R[None], t[None], kp[None], X[None], conf[None])
    assert base["keep"].all() and base["report"][0].tolist()[2:] == [1.0, 1.0, 6.0] and base["em"].max() < 1e-9
    # joint 1 behind camera 1 only (its keypoints follow, so its error stays zero)
    Xb = X.copy()
    Xb[1] = [-3.0, 0.0, 0.2]
    kpb = kp.copy()
    for v in range(2):
        p = (Xb[1] @ R[v].T + t[v]) @ K[v].T
        kpb[v, 1] = p[:2] / p[2]
    r = ref.triage(K[None], R[None], t[None], kpb[None], Xb[None], conf[None])
    assert r["depth"][0, 0, 1] > 0 > r["depth"][0, 1, 1] and r["em"][0, 1] < 1e-6
    assert r["keep"][0].tolist() == [True, False, True, True, True, True] and r["report"][0, 2] == 5 / 6
    # joint 2: 3 px off in one view -> em = 1.5 passes; 5 px -> em = 2.5 fails
    for off, ok in ((3.0, True), (5.0, False)):
        kpe = kp.copy()
        kpe[0, 2, 0] += off
        r = ref.triage(K[None], R[None], t[None], kpe[None], X[None], conf[None])
        assert abs(r["em"][0, 2] - off / 2) < 1e-9 and bool(r["keep"][0, 2]) is ok and r["pos"].all()
    # joint 3: a low score in one view
    c2 = conf.copy()
    c2[1, 3] = 0.29
    r = ref.triage(K[None], R[None], t[None], kp[None], X[None], c2[None])
    assert r["keep"][0].tolist() == [True, True, True, False, True, True]
    assert np.isnan(r["X_clean"][0, 3]).all() and np.array_equal(r["X_clean"][0, 4], X[4])
    assert ref.triage(K[None], R[None], t[None], kp[None], X[None], None)["keep"].all()
    # a NaN keypoint: its error is NaN, the joint is dropped, the statistics ignore it
    kpn = kp.copy()
    kpn[0, 5, 1] = np.nan
    r = ref.triage(K[None], R[None], t[None], kpn[None], X[None], conf[None])
    assert np.isnan(r["err"][0, 0, 5]) and not r["keep"][0, 5] and np.isfinite(r["view_stats"]).all()


def test_two_view_triage_matches_the_references_post_triage_sequence(golden_dir):
    """tests/golden/post_triage.npz: inputs and outputs of the reference's own post_triage_sequence
    (tools/make_goldens.py post_triage; a 12-step two-view clip with joints behind a camera, a NaN keypoint, outliers
    and low scores).  Its cameras are K1 [I | 0] and K2 [R | T], so the V = 2 restatement with view 0 at the origin must
    give its keep masks exactly and its reports to 1e-9 (1 + |x|) (the reference adds 1e-12 to the depth before it
    divides: < 1e-9 px here); the smoothed joints to float32 rounding, the format the reference stores them in."""
    g = np.load(golden_dir / "post_triage.npz")
    Tn = g["X"].shape[0]
    K = np.broadcast_to(np.stack([g["K1"], g["K2"]]), (Tn, 2, 3, 3))
    R = np.broadcast_to(np.stack([np.eye(3), g["R"]]), (Tn, 2, 3, 3))
    t = np.broadcast_to(np.stack([np.zeros(3), g["T"]]), (Tn, 2, 3))
    kp = np.stack([g["kL"], g["kR"]], axis=1)
    conf = np.stack([g["confL"], g["confR"]], axis=1)
    for tag, c in (("conf", conf), ("noconf", None)):
        r = ref.triage(K, R, t, kp, g["X"], c, float(g["conf_thr"]), float(g["err_thresh_px"]))
        want_keep = ~np.isnan(g[f"{tag}_X_clean"]).all(axis=-1)
        assert 0 < want_keep.sum() < want_keep.size and np.array_equal(r["keep"], want_keep), tag
        assert np.array_equal(r["X_clean"].astype(np.float32), g[f"{tag}_X_clean"], equal_nan=True)
        assert (np.abs(r["report"] - g[f"{tag}_report"]) <= 1e-9 * (1 + np.abs(g[f"{tag}_report"]))).all(), tag
    sm = fuse.smooth_skeleton(g["conf_X_clean"], win=int(g["sg_win"]))
    want = g["conf_X_clean_smoothed"]
    assert np.array_equal(np.isnan(sm), np.isnan(want)) and not np.array_equal(want, g["conf_X_clean"], equal_nan=True)
    assert np.nanmax(np.abs(sm - want) / (1 + np.abs(want))) <= 2.0 ** -23


def test_recenter_restatement_is_recenter_and_align():
    rng = np.random.default_rng(5)
    from scipy.spatial.transform import Rotation
    R = Rotation.from_rotvec(rng.normal(scale=0.3, size=(2, 3))).as_matrix()
    t = rng.normal(size=(2, 3))
    o = rng.normal(size=(2, 3))
    origin, R2, t2 = ref.recenter(o, [5, 9], R, t)
    Rw, tw = mv.recenter_and_align(R, t, 0.5 * (o[0] + o[1]))
    assert np.array_equal(origin, 0.5 * (o[0] + o[1])) and np.array_equal(R2, Rw) and np.array_equal(t2, tw)
    assert np.array_equal(t2[1], t[1] + R[1] @ origin)        # the turn-then-mirror leaves t_1 where the recentring put it
    origin, R3, t3 = ref.recenter(o, [5, 0], R, t)
    assert not origin.any() and np.array_equal(t3, t)
    origin, R4, _ = ref.recenter(np.concatenate([o, o[:1]]), [1, 1, 1], np.concatenate([R, R[:1]]), np.concatenate([t, t[:1]]))
    assert np.array_equal(R4[1], R[1]) and np.allclose(origin, (2 * o[0] + o[1]) / 3)


def test_gpu_case_margins():
    """the maps of tests/test_person_gpu.py satisfy its margin condition (checked here, where no GPU is needed)"""
    import test_person_gpu as g
    for name, P, boxes, src in g.person_cases():
        for m in range(len(P)):
            r = ref.person_origin(P[m], boxes[m], src)
            assert ref.margin(r) > 1e-6, (name, m, ref.margin(r))


def test_new_entry_points_reject_host_tensors_and_bad_arguments():
    lib = _lib.lib()
    assert lib.skimi_person_workspace_bytes(8, 518, 518) == 0
    d = ctypes.c_void_p(16)
    assert lib.skimi_person_origin(d, d, 0, 518, 518, 1080, 1920, None, d, None) != 0
    assert lib.skimi_person_origin(d, d, 1, 518, 518, 0, 1920, None, d, None) != 0
    assert lib.skimi_person_origin(None, d, 1, 518, 518, 1080, 1920, None, d, None) != 0
    assert b"skimi_person_origin" in lib.skimi_last_error()
    assert lib.skimi_recenter_cameras(d, d, 1, 9, d, d, d, None) != 0
    for V, J in ((1, 17), (9, 17), (2, 0), (2, 33)):
        assert lib.skimi_triangulate_triage(d, d, d, d, None, 0.3, 2.0, 1, V, J, d, d, d, d, d, d, d, None) != 0
    assert b"2..8 views" in lib.skimi_last_error()
    with pytest.raises(_lib.SkimiError, match="device"):
        geometry.person_origin(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4), (4, 4))
    with pytest.raises(_lib.SkimiError, match="device"):
        geometry.triangulate_triage(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3), torch.zeros(1, 2, 17, 2))
    with pytest.raises(_lib.SkimiError, match="device"):
        geometry.recenter_cameras(torch.zeros(1, 2, 8, dtype=torch.float64), torch.zeros(1, 2, 3, 4))


def test_clip_path_rejects_host_or_misshapen_inputs_before_any_launch():
    """boxes, keypoints and scores reach the kernels as raw pointers: a host tensor or a wrong shape is an error, not a
    fault (the model is never called: None stands in for it)"""
    from skiing_analysis_pytorch_amd import infer
    T, S, J = 3, 2, 17
    frames = torch.zeros(T, S, 3, 28, 28)
    kp, boxes, scores = torch.zeros(T, S, J, 2), torch.zeros(T, S, 4), torch.zeros(T, S, J)
    with pytest.raises(ValueError, match="boxes must be a device tensor"):
        infer.process_multi_view_clip(None, frames, kp, boxes=boxes)
    with pytest.raises(ValueError, match="keypoints must be a device tensor"):
        infer.process_multi_view_clip(None, frames, kp, triage=True)
    with pytest.raises(ValueError, match="scores are only read by triage"):
        infer.process_multi_view_clip(None, frames, kp, scores=scores)
    if torch.cuda.is_available():
        kd = kp.cuda()
        with pytest.raises(ValueError, match="scores must be a device tensor"):
            infer.process_multi_view_clip(None, frames, kd, scores=scores, triage=True)
        with pytest.raises(ValueError, match="scores must be a device tensor"):
            infer.process_multi_view_clip(None, frames, kd, scores=torch.zeros(T, J).cuda(), triage=True)
        with pytest.raises(ValueError, match="keypoints must be a device tensor"):
            infer.process_multi_view_clip(None, frames, kd[:, :1], triage=True)
