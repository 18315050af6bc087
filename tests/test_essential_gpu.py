"""GPU: the essential-matrix RANSAC (csrc/essential.hip: prep, hypotheses, score and finish kernels, five_point_kernel;
geometry.essential_ransac, geometry.five_point, run.solve_rt_from_essential, camera_position) against the float64
restatement tests/essential_restated.py on the inputs of tests/essential_cases.py.

Bounds: the integer outputs (n_used, inliers, pose_mask, cheirality, winner, n_solutions, success) equal; E, R, t, cost and
confidence within 1e-9 (1 + |x|), the project's float64 tolerance, on the cases tests/test_essential_cpu.py shows to be
stable (the winner leads, no point sits on the threshold, a 1e-13 change of the keypoints moves the pose by <= 1e-10); the
noise-free cases, whose costs are rounding, against the true pose with the CPU test's POSE_BOUND (9.0e-14)."""
import numpy as np
import pytest
import torch

import essential_cases as ec
import essential_restated as er
import resect_cases as rc
import test_essential_cpu as tc
from skiing_analysis_pytorch_amd import _lib, camera_position, geometry, run

dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
INT_KEYS = ("n_used", "n_inliers", "n_pose", "cheirality", "winner", "n_solutions", "success")
FLOAT_KEYS = ("E", "R", "t", "cost", "confidence")
COMPARED = [c[0] for c in ec.comparison_cases()] + ["masked_T8_step"]


def _close(got, want, what, tol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isnan(want) | (got == want) | (np.abs(got - want) <= tol * (1 + np.abs(want)))
    assert ok.all(), (what, float(np.nanmax(np.abs(got - want))))
    return float(np.nanmax(np.abs(got - want) / (1 + np.abs(want)), initial=0.0))


def kernel(p, kw, sl=None, **more):
    x2d, conf = p["x2d"], p["conf"]
    if sl is not None:
        x2d, conf = x2d[:, sl], None if conf is None else conf[:, sl]
    r = geometry.essential_ransac(dev(x2d), dev(p["K"]), conf=dev(conf), **dict(kw, **more))
    assert r.success.dtype == torch.bool and r.inliers.dtype == torch.uint8 and r.R.dtype == torch.float64
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def _problem(name):
    return ec.masked_case()[1:3] if name == "masked_T8_step" else ec.case(name)[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", COMPARED)
def test_kernel_matches_restatement(name):
    p, kw = _problem(name)
    got, want = kernel(p, kw), ec.restated(name)
    G = len(want["n_used"])
    gs = kw["group_size"] or p["x2d"].shape[1]
    groups = [g for g in range(G) if name != "masked_T8_step" or g != ec.MASKED_FIVE]
    g = np.array(groups)
    for k in INT_KEYS:
        assert np.array_equal(got[k][g], want[k][g].astype(got[k].dtype)), (name, k, got[k], want[k])
    cols = (g[:, None] * gs + np.arange(gs)[None]).ravel()
    for k in ("inliers", "pose_mask"):
        assert np.array_equal(got[k][cols], want[k][cols]), (name, k)
    worst = {k: _close(got[k][g], want[k][g], f"{name}: {k}") for k in FLOAT_KEYS}
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    if name == "masked_T8_step":                         # exactly five used points: every sample is those five and fits them
        f = ec.MASKED_FIVE
        assert got["n_used"][f] == 5 and got["n_inliers"][f] == 5 and got["success"][f] and got["cost"][f] <= 1e-20
        d = want["details"][f]
        e2 = er.sampson(got["E"][f], d["a"], d["b"])
        assert e2.max() <= 1e-20, e2
        f = ec.MASKED_FAILED
        assert got["n_used"][f] == 4 and not got["success"][f] and np.isnan(got["R"][f]).all() and tuple(got["winner"][f]) == (-1, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in ec.clean_cases()])
def test_noise_free_pose_is_the_rigs(name):
    _, p, kw = ec.case(name)
    got = kernel(p, kw)
    assert got["success"].all() and (got["n_inliers"] == got["n_used"]).all() and (got["n_pose"] == got["n_used"]).all()
    assert got["inliers"].all() and got["pose_mask"].all()
    eR, et = np.abs(got["R"] - p["R"]).max(), np.abs(got["t"] - p["t"]).max()
    eE = np.abs(got["E"] - er.skew(p["t"]) @ p["R"]).max()
    print(name, "R", eR, "t", et, "E", eE)
    assert max(eR, et, eE) <= tc.POSE_BOUND


@pytest.mark.gpu
def test_five_point_kernel_matches_restatement():
    a, b = ec.solver_samples()
    E, counts, d = ec.solver_restated()
    Eg, cg = geometry.five_point(dev(a), dev(b))
    Eg, cg = Eg.cpu().numpy(), cg.cpu().numpy()
    assert cg.dtype == np.int32 and np.array_equal(cg, counts)
    assert np.array_equal(np.isnan(Eg), np.isnan(E))
    # the samples on which the two eigen-solves must agree: solutions pairwise more than 1e-4 apart, and no discarded
    # eigenvalue closer than 1e-6 to the real axis
    stable = np.ones(len(counts), bool)
    for s in range(len(counts)):
        sols = E[s, :counts[s]].reshape(counts[s], 9)
        if counts[s] > 1:
            dist = np.sqrt(((sols[:, None] - sols[None]) ** 2).sum(axis=-1))[np.triu_indices(counts[s], 1)]
            stable[s] &= bool(dist.min() > 1e-4)
        if d["ok"][s]:
            w = np.linalg.eigvals(d["A"][s])
            stable[s] &= bool((np.abs(w.imag[w.imag != 0.0]) > 1e-6).all())
    left_out = 1.0 - stable.mean()
    worst = np.nanmax(np.abs(Eg - E)[stable])
    print("five_point: worst", worst, "over", int(stable.sum()), "samples;", f"{100 * left_out:.1f} % left out;",
          "worst over all", np.nanmax(np.abs(Eg - E)))
    assert left_out <= 0.05
    assert worst <= 1e-8


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise1_T8_step", "conf_T8_step", "out10_T64_clip", "masked_T8_step"])
def test_rerun_and_group_slices_are_bitwise_equal(name):
    """every sum has a fixed order that depends only on a point's rank within its group, and the samples only on
    (seed, group + group_offset, hypothesis)"""
    p, kw = _problem(name)
    full, again = kernel(p, kw), kernel(p, kw)
    for k in full:
        assert np.array_equal(full[k], again[k], equal_nan=True), (name, k, "rerun")
    if kw["group_size"] is None:
        return
    G, J = len(full["n_used"]), ec.J
    for lo, hi in ((0, 2), (3, G), (5, 6)):
        part = kernel(p, kw, sl=slice(lo * J, hi * J), group_offset=lo)
        for k in full:
            ref = full[k][lo * J:hi * J] if k in ("inliers", "pose_mask") else full[k][lo:hi]
            assert np.array_equal(part[k], ref, equal_nan=True), (name, k, lo, hi)


@pytest.mark.gpu
def test_bad_arguments_raise_before_a_launch():
    _, p, kw = ec.case("noise1_T8_step")
    x2d, K = dev(p["x2d"]), dev(p["K"])
    for bad in (dict(hypotheses=0), dict(hypotheses=65537), dict(group_size=0), dict(group_size=16), dict(group_size=x2d.shape[1] + 1),
                dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan"))):
        with pytest.raises(_lib.SkimiError):
            geometry.essential_ransac(x2d, K, **dict(dict(group_size=ec.J, hypotheses=16), **bad))
    with pytest.raises(_lib.SkimiError):
        geometry.essential_ransac(x2d.cpu(), K)
    with pytest.raises(_lib.SkimiError):
        geometry.five_point(torch.zeros(4, 5, 2, dtype=torch.float64), torch.zeros(4, 5, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        geometry.essential_ransac(x2d[0], K)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_solve_rt_from_essential(tmp_path):
    c = rc.rig(T=64, V=2, seed=47, noise=1.0)
    X, x2d, _ = rc.flat(c)
    args = dict(K_left=c["K"][0], K_right=c["K"][1], hypotheses=256, seed=4103)
    out = tmp_path / "rt" / "essential.npz"
    init = run.solve_rt_from_essential(c["X"], c["x2d"][0], c["x2d"][1], refine="none", out=out, **args)
    assert set(np.load(out).files) == set(run.RT_KEYS) | {"inliers"}
    e = geometry.essential_ransac(dev(x2d), dev(c["K"]), hypotheses=256, seed=4103)
    assert np.array_equal(init["RL"], np.eye(3)) and np.array_equal(init["tL"], np.zeros(3))
    assert np.array_equal(init["RR"], e.R[0].cpu().numpy()) and np.array_equal(init["tR"], e.t[0].cpu().numpy())
    assert np.array_equal(init["R_rel"], init["RR"]) and np.array_equal(init["inliers"], e.inliers.bool().cpu().numpy())
    assert init["inliers"].shape == (X.shape[0],) and init["n_points"] == X.shape[0] and init["success"] == 1
    # refine="camera" ends where resect_cameras ends from the same start
    res = run.solve_rt_from_essential(c["X"], c["x2d"][0], c["x2d"][1], refine="camera", **args)
    R0 = torch.stack([torch.eye(3, dtype=torch.float64).cuda(), e.R[0]])[None]
    t0 = torch.stack([torch.zeros(3, dtype=torch.float64).cuda(), e.t[0]])[None]
    r = geometry.resect_cameras(dev(X), dev(x2d), K=dev(c["K"]), R0=R0, t0=t0)
    assert np.array_equal(res["RR"], r.R[0, 1].cpu().numpy()) and np.array_equal(res["tL"], r.t[0, 0].cpu().numpy())
    assert res["mean_err_R"] == float(r.mean_err[0, 1]) and res["mean_err_R"] < init["mean_err_R"]
    with pytest.raises(ValueError):
        run.solve_rt_from_essential(c["X"], c["x2d"][0], c["x2d"][1], K_left=c["K"][0])
    with pytest.raises(NotImplementedError, match="solve_rt_from_essential"):
        run.solve_rt_from_3d(c["X"], c["x2d"][0], c["x2d"][1], init="essential")


@pytest.mark.gpu
def test_estimate_camera_pose_from_kpt():
    _, p, kw = ec.case("noise1_T8_step")
    K, J = p["K"][0], ec.J
    pts1, pts2 = p["x2d"][0].reshape(-1, J, 2), p["x2d"][1].reshape(-1, J, 2)
    R, T, mask_pose = camera_position.estimate_camera_pose_from_kpt(pts1[0], pts2[0], K, 2.5, hypotheses=256)
    assert R.shape == (3, 3) and T.shape == (3, 1) and mask_pose.shape == (J,) and mask_pose.dtype == np.uint8
    assert abs(np.linalg.norm(-R.T @ T) - 2.5) <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
    assert camera_position.estimate_camera_pose_from_kpt(pts1[0, :4], pts2[0, :4], K, 2.5, hypotheses=16) == (None, None, None)
    assert camera_position.estimate_camera_pose_from_kpt(pts1[0, :0], pts2[0, :0], K, 2.5) == (None, None, None)
    Rs, Ts, masks, ok = camera_position.estimate_camera_poses_from_kpts(pts1, pts2, K, 2.5, hypotheses=256)
    assert Rs.shape == (8, 3, 3) and Ts.shape == (8, 3, 1) and masks.shape == (8, J) and ok.shape == (8,) and ok.all()
    assert np.array_equal(Rs[0], R) and np.array_equal(Ts[0], T) and np.array_equal(masks[0], mask_pose)
    for f in (3, 7):                # a frame alone with its group_offset is bitwise the frame of the batch
        Rf, Tf, mf = camera_position.estimate_camera_pose_from_kpt(pts1[f], pts2[f], K, 2.5, hypotheses=256, group_offset=f)
        assert np.array_equal(Rs[f], Rf) and np.array_equal(Ts[f], Tf) and np.array_equal(masks[f], mf)
    assert np.abs(np.linalg.norm(Ts[:, :, 0], axis=1) - 2.5).max() <= 1e-12
