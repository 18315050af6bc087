"""GPU: the camera resection (csrc/resect.hip: resect_kernel, relative_pose_kernel; geometry.resect_cameras,
run.solve_rt_from_3d) against the float64 restatement tests/resect_restated.py on the inputs of tests/resect_cases.py.

Bounds: n_points and success equal, NaN patterns equal; R, t, K, err, the costs and the statistics within
1e-9 (1 + |x|), the project's float64 tolerance (tests/test_resect_cpu.py shows that the stopping point moves by 4e-13
under a 1e-13 change of the start, so what is left between kernel and restatement is the order of their sums).
Measured on an MI355X: worst 3.9e-12 in R, 3.6e-11 in err (17-point problems with gross outliers), 4e-15 and 3.4e-13
on every other case."""
import numpy as np
import pytest
import torch

import resect_cases as rc
import resect_restated as rr
import robust_restated as rob
from skiing_analysis_pytorch_amd import _lib, geometry, run

dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
FLOAT_KEYS = ("R", "t", "K", "cost0", "cost", "mean_err", "rms_err", "max_err", "R_rel", "t_rel")
ALL = rc.cases() + [rc.given_start_case()[:4], rc.masked_case()[:4]]


def _close(got, want, what, tol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isnan(want) | (got == want) | (np.abs(got - want) <= tol * (1 + np.abs(want)))
    assert ok.all(), (what, float(np.nanmax(np.abs(got - want))))
    return float(np.nanmax(np.abs(got - want) / (1 + np.abs(want)), initial=0.0))


def kernel(X, x2d, conf, kw):
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = geometry.resect_cameras(dev(X), dev(x2d), conf=dev(conf), **kw)
    assert r.success.dtype == torch.bool and r.n_points.dtype == torch.int32 and r.R.dtype == torch.float64
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_kernel_matches_restatement(case):
    name, c, kw, groups = case
    X, x2d, conf = rc.flat(c)
    got = kernel(X, x2d, conf, kw)
    want = rr.resect_cameras(X, x2d, conf=conf, groups=groups, **kw)
    g = np.array(groups)
    gs = kw["group_size"] or X.shape[0]
    assert np.array_equal(got["n_points"][g], want["n_points"][g]), name
    assert np.array_equal(got["success"][g], want["success"][g].astype(bool)), name
    worst = {k: _close(got[k][g], want[k][g], f"{name}: {k}") for k in FLOAT_KEYS}
    cols = (g[:, None] * gs + np.arange(gs)[None]).ravel()
    worst["err"] = _close(got["err"][:, cols], want["err"][:, cols], f"{name}: err")
    print(name, {k: f"{v:.1e}" for k, v in worst.items()}, "n_evals equal:", np.array_equal(got["n_evals"][g], want["n_evals"][g]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise1_T64_V2_step_conf", "out10_T64_V2_step_soft_l1", "inferK_T64_V3_step_conf",
                                  "clean_T1024_V3_step"])
def test_a_group_is_bitwise_what_it_is_alone_and_on_a_rerun(name):
    """every sum's order depends only on a point's index within its group"""
    _, c, kw, groups = next(x for x in ALL if x[0] == name)
    X, x2d, conf = rc.flat(c)
    full = kernel(X, x2d, conf, kw)
    again = kernel(X, x2d, conf, kw)
    for k in full:
        assert np.array_equal(full[k], again[k], equal_nan=True), (name, k, "rerun")
    for g in groups[:6]:
        sl = slice(g * rc.J, (g + 1) * rc.J)
        alone = kernel(X[sl], x2d[:, sl], None if conf is None else conf[:, sl], kw)
        for k in full:
            a, b = (alone[k][:, :], full[k][:, sl]) if k == "err" else (alone[k][0], full[k][g])
            assert np.array_equal(a, b, equal_nan=True), (name, g, k)


@pytest.mark.gpu
def test_whole_clip_problem_is_bitwise_reproducible_and_independent_of_the_other_views():
    _, c, kw, _ = next(x for x in ALL if x[0] == "out10_T64_V3_clip_conf_soft_l1")
    X, x2d, conf = rc.flat(c)
    a, b = kernel(X, x2d, conf, kw), kernel(X, x2d, conf, kw)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    # views 0 and 1 alone: the mask still comes from every view given, so drop view 2 only where it masks nothing
    two = kernel(X, x2d[:2], conf[:2], dict(kw, K=kw["K"][:2]))
    for k in ("R", "t", "cost", "n_evals"):
        assert np.array_equal(two[k][0], a[k][0, :2]), k


@pytest.mark.gpu
def test_masked_points_equal_their_removal():
    name, c, kw, groups, n_points = rc.masked_case()
    X, x2d, conf = rc.flat(c)
    full = kernel(X, x2d, conf, kw)
    assert np.array_equal(full["n_points"], np.stack([n_points, n_points], axis=1))
    assert np.array_equal(full["success"][:, 0], n_points >= rr.MIN_POINTS)
    _, used = rr.weights_and_mask(X, x2d, conf, rc.MIN_CONF)
    for g in (0, 3, 4, 6):
        keep = np.zeros(X.shape[0], bool)
        keep[g * rc.J:(g + 1) * rc.J] = used[g * rc.J:(g + 1) * rc.J]
        assert keep.sum() == 16
        Xr, xr, cr = rc.removed(c, keep)
        alone = kernel(Xr, xr, cr, dict(kw, group_size=None))
        for k in FLOAT_KEYS:
            _close(alone[k][0], full[k][g], f"group {g}: {k}")
        _close(alone["err"], full["err"][:, keep], f"group {g}: err")


@pytest.mark.gpu
def test_relative_pose_matches_the_formulas():
    rng = np.random.default_rng(5)
    G, V = 7, 3
    R = np.stack([[rr.exp_so3(rng.normal(0, 1, 3)) for _ in range(V)] for _ in range(G)])
    t = rng.normal(0, 3, (G, V, 3))
    R[2, 1, 0, 0] = np.nan
    R_rel, t_rel = geometry.relative_pose(dev(R), dev(t))
    for g in range(G):
        want_R, want_t = rr.relative_pose(R[g], t[g])
        _close(R_rel[g].cpu().numpy(), want_R, "R_rel", 1e-14)
        _close(t_rel[g].cpu().numpy(), want_t, "t_rel", 1e-14)
    assert np.abs(R_rel[:, 0].cpu().numpy() - np.eye(3)).max() < 1e-14 and np.abs(t_rel[:, 0].cpu().numpy()).max() < 1e-14


@pytest.mark.gpu
def test_solve_rt_from_3d_writes_the_references_keys(tmp_path):
    name, c, kw, groups, n_points = rc.masked_case()
    out = tmp_path / "sub" / "rt_result.npz"
    res = run.solve_rt_from_3d(c["X"], c["x2d"][0], c["x2d"][1], conf_left=c["conf"][0], conf_right=c["conf"][1],
                               K_left=c["K"][0], K_right=c["K"][1], huber=2.0, min_conf=rc.MIN_CONF, out=out)
    z = np.load(out)
    assert sorted(z.files) == sorted(["RL", "tL", "RR", "tR", "R_rel", "t_rel", "K_L", "K_R", "mean_err_L", "median_err_L",
                                      "mean_err_R", "median_err_R", "success", "n_points"])
    assert int(z["n_points"]) == int(n_points.sum()) == res["n_points"] and int(z["success"]) == 1
    X, x2d, conf = rc.flat(c)
    want = rr.resect_cameras(X, x2d, K=c["K"], conf=conf, loss="soft_l1", f_scale=2.0, min_conf=rc.MIN_CONF)
    for key, w in (("RL", want["R"][0, 0]), ("tL", want["t"][0, 0]), ("RR", want["R"][0, 1]), ("tR", want["t"][0, 1]),
                   ("R_rel", want["R_rel"][0, 1]), ("t_rel", want["t_rel"][0, 1]), ("K_L", c["K"][0]), ("K_R", c["K"][1]),
                   ("mean_err_L", want["mean_err"][0, 0]), ("mean_err_R", want["mean_err"][0, 1]),
                   ("median_err_L", np.nanmedian(want["err"][0])), ("median_err_R", np.nanmedian(want["err"][1]))):
        _close(z[key], w, key)
    assert z["RL"].shape == (3, 3) and z["t_rel"].shape == (3,) and z["mean_err_L"].shape == ()
    # one K absent: inferred from that view's masked keypoints, the other kept
    one = run.solve_rt_from_3d(c["X"], c["x2d"][0], c["x2d"][1], conf_left=c["conf"][0], conf_right=c["conf"][1],
                               K_left=c["K"][0], min_conf=rc.MIN_CONF)
    _, used = rr.weights_and_mask(X, x2d, conf, rc.MIN_CONF)
    _close(one["K_R"], rr.infer_K(x2d[1][used]), "inferred K_R")
    assert np.array_equal(one["K_L"], c["K"][0])
    # refine="none" is the start; what is out of scope says so
    start = run.solve_rt_from_3d(X, x2d[0], x2d[1], K_left=c["K"][0], K_right=c["K"][1], refine="none")
    w0 = rr.resect_cameras(X, x2d, K=c["K"], max_evals=1)
    _close(start["RL"], w0["R"][0, 0], "start RL")
    _close(start["tR"], w0["t"][0, 1], "start tR")
    assert start["success"] == 1
    for bad in (dict(init="essential"), dict(refine="camera_points")):
        with pytest.raises(NotImplementedError, match="DESIGN"):
            run.solve_rt_from_3d(X, x2d[0], x2d[1], **bad)


@pytest.mark.gpu
def test_recovered_cameras_triangulate_the_points_back():
    """noise-free, per step: resect_cameras -> geometry.triangulate_joints with the recovered cameras.  The DLT kernel
    takes float32 cameras and keypoints, so what it can return is the float64 DLT of those float32 inputs (the
    restatement of tests/robust_restated.py) to one float32 ulp, the bound tests/test_robust_gpu.py uses; that point is
    X up to the rounding of the inputs (1e-5: a float32 keypoint near 1100 px is 6e-5 px off, a t near 4.5 is 2e-7 off)."""
    _, c, kw, _ = next(x for x in ALL if x[0] == "clean_T64_V3_step")
    X, x2d, conf = rc.flat(c)
    r = geometry.resect_cameras(dev(X), dev(x2d), K=dev(c["K"]), group_size=rc.J)
    assert bool(r.success.all())
    T, V = c["T"], c["V"]
    K32, R32, t32 = r.K.float(), r.R.float(), r.t.float()
    kp32 = dev(c["x2d"].transpose(1, 0, 2, 3)).float()                    # [T, V, J, 2]
    got = geometry.triangulate_joints(K32, R32, t32, kp32).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (T, rc.J, 3)
    Kn, Rn, tn, kn = (a.cpu().numpy().astype(np.float64) for a in (K32, R32, t32, kp32))
    for ti in range(T):
        P = rob.cameras(Kn[ti], Rn[ti], tn[ti])
        for j in range(rc.J):
            w32 = rob.dlt(P, kn[ti, :, j], range(V))[0].astype(np.float32)
            assert (np.abs(got[ti, j] - w32) <= np.spacing(np.abs(w32))).all(), (ti, j)
    assert np.abs(got - c["X"]).max() <= 1e-5


@pytest.mark.gpu
def test_cpu_tensors_and_bad_shapes_are_rejected():
    c = rc.rig(T=2, V=2, seed=1)
    X, x2d, _ = rc.flat(c)
    with pytest.raises(_lib.SkimiError, match="device tensors"):
        geometry.resect_cameras(torch.from_numpy(X), torch.from_numpy(x2d))
    with pytest.raises(_lib.SkimiError, match="device tensors"):
        geometry.relative_pose(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3))
    with pytest.raises(ValueError):
        geometry.resect_cameras(dev(X), dev(x2d[:, :-1]))
    with pytest.raises(ValueError):
        geometry.resect_cameras(dev(X), dev(x2d), loss="huber")
    with pytest.raises(_lib.SkimiError, match="does not divide"):
        geometry.resect_cameras(dev(X), dev(x2d), group_size=5)


@pytest.mark.gpu
def test_bad_arguments_return_an_error_code_without_a_launch():
    lib = _lib.lib()
    c = rc.rig(T=2, V=2, seed=1)
    X, x2d, _ = rc.flat(c)
    N = X.shape[0]
    Xd, xd = dev(X), dev(x2d)
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")    # noqa: E731
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")        # noqa: E731
    outs = [f64(1, 2, 3, 3), f64(1, 2, 3), f64(1, 2, 3, 3), f64(1, 2), f64(1, 2), i32(1, 2), i32(1, 2), i32(1, 2), f64(2, N), f64(1, 2, 3)]

    def call(X=Xd, x2d=xd, R0=None, t0=None, n=N, views=2, gs=N, loss=0, f_scale=1.0, max_evals=200, outs=outs):
        p = [None if o is None else o.data_ptr() for o in outs]
        return lib.skimi_resect_cameras(_lib.ptr(X), _lib.ptr(x2d), None, None, _lib.ptr(R0), _lib.ptr(t0), n, views, gs, loss,
                                        f_scale, 0.0, max_evals, *p, None, 0, None)

    for kw, msg in ((dict(gs=5), b"does not divide"), (dict(gs=0), b"does not divide"), (dict(views=0), b"views"),
                    (dict(views=9), b"views"), (dict(X=None), b"NULL input"), (dict(x2d=None), b"NULL input"),
                    (dict(outs=[None] + outs[1:]), b"NULL output"), (dict(outs=outs[:-1] + [None]), b"NULL output"),
                    (dict(R0=f64(1, 2, 3, 3)), b"go together"), (dict(loss=2), b"unknown loss"), (dict(f_scale=0.0), b"f_scale"),
                    (dict(max_evals=0), b"max_evals"), (dict(n=0), b"does not divide"),
                    (dict(n=800_000_000, gs=800_000_000), b"32-bit point offsets")):
        assert call(**kw) == -1, kw                      # SKIMI_ERR_ARG
        assert msg in lib.skimi_last_error(), (kw, lib.skimi_last_error())
    assert lib.skimi_relative_pose(None, None, 1, 2, None, None, None) == -1 and b"NULL" in lib.skimi_last_error()
    assert lib.skimi_relative_pose(outs[0].data_ptr(), outs[1].data_ptr(), 1, 0, outs[0].data_ptr(), outs[1].data_ptr(), None) == -1
    assert lib.skimi_resect_workspace_bytes(N, 2, N) == 0
    torch.cuda.synchronize()
    for o in outs:                                       # nothing was launched: the outputs are untouched
        assert bool((o == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert int(outs[6][0, 0]) == N
