"""GPU: the camera-and-points refinement (csrc/refine.hip: refine_kernel; geometry.refine_cameras_points,
run.solve_rt_and_points) against the float64 restatement tests/refine_restated.py on the inputs of tests/refine_cases.py.

Bounds: n_points and success equal, NaN patterns equal; with lambda_x > 0 R, t, K, X_opt, err, the costs and the statistics
within 1e-9 (1 + |x|), the project's float64 tolerance (tests/test_refine_cpu.py shows that the stopping point of those
cases moves by under 1e-10 when the start moves by 1e-13 relative, so what is left between kernel and restatement is the
order of their sums); with lambda_x = 0 the gauge-invariant outputs only: costs, err and the statistics (rule 9)."""
import numpy as np
import pytest
import torch

import refine_cases as fc
import refine_restated as fr
import resect_restated as rr
from skiing_analysis_pytorch_amd import _lib, geometry, run

dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
INVARIANT_KEYS = ("K", "cost0", "cost", "mean_err", "rms_err", "max_err")
GAUGE_KEYS = ("R", "t", "X_opt", "moved", "R_rel", "t_rel")
ALL = fc.cases()


def _close(got, want, what, tol=1e-9):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isnan(want) | (got == want) | (np.abs(got - want) <= tol * (1 + np.abs(want)))
    assert ok.all(), (what, float(np.nanmax(np.abs(got - want))))
    return float(np.nanmax(np.abs(got - want) / (1 + np.abs(want)), initial=0.0))


def kernel(X, x2d, conf, kw):
    kw = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    r = geometry.refine_cameras_points(dev(X), dev(x2d), conf=dev(conf), **kw)
    assert r.success.dtype == torch.bool and r.n_points.dtype == torch.int32 and r.X_opt.dtype == torch.float64
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


_WANT = {}


def restated(name):
    """the restatement's result of a case, computed once"""
    if name not in _WANT:
        _, c, kw = next(x for x in ALL if x[0] == name)
        X, x2d, conf = fc.flat(c)
        _WANT[name] = fr.refine_cameras_points(X, x2d, conf=conf, **kw)
    return _WANT[name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL, ids=lambda c: c[0])
def test_kernel_matches_restatement(case):
    """n = 6 (the minimum), 17-point per-step groups at V = 1, 2, 3, 4 (every shape of the Schur chunks), n = 65 (two
    waves), n = 1100 (the strided path: more points than the 512 threads of a workgroup); both losses, K given and inferred, with and without scores"""
    name, c, kw = case
    X, x2d, conf = fc.flat(c)
    got, want = kernel(X, x2d, conf, kw), restated(name)
    assert np.array_equal(got["n_points"], want["n_points"]), name
    assert np.array_equal(got["success"], want["success"].astype(bool)), name
    keys = INVARIANT_KEYS + ("err",) + (GAUGE_KEYS if kw["lambda_x"] > 0 else ())
    worst = {k: _close(got[k], want[k], f"{name}: {k}") for k in keys}
    print(name, {k: f"{v:.1e}" for k, v in worst.items()}, "n_evals equal:", np.array_equal(got["n_evals"], want["n_evals"]))
    if kw["lambda_x"] > 0:
        assert got["success"].all(), name                   # rule 9 (a): stopped on the step criterion


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["step_V2_lx1", "step_V3_lx0_conf", "step_V4_lx100_inferK", "step_V1_lx1"])
def test_a_group_is_bitwise_what_it_is_alone_in_a_batch_and_on_a_rerun(name):
    """every sum's order depends only on a point's index within its group"""
    _, c, kw = next(x for x in ALL if x[0] == name)
    X, x2d, conf = fc.flat(c)
    full, again = kernel(X, x2d, conf, kw), kernel(X, x2d, conf, kw)
    for k in full:
        assert np.array_equal(full[k], again[k], equal_nan=True), (name, k, "rerun")
    for g in (0, 3):
        sl = slice(g * fc.J, (g + 1) * fc.J)
        alone = kernel(X[sl], x2d[:, sl], None if conf is None else conf[:, sl], dict(kw, R0=kw["R0"][g:g + 1], t0=kw["t0"][g:g + 1]))
        for k in full:
            a, b = (alone[k], full[k][:, sl]) if k == "err" else (alone[k], full[k][sl]) if k == "X_opt" else (alone[k][0], full[k][g])
            assert np.array_equal(a, b, equal_nan=True), (name, g, k)


@pytest.mark.gpu
def test_whole_clip_groups_are_bitwise_reproducible():
    for name in ("n65_V2_lx1", "n1100_V2_lx0"):
        _, c, kw = next(x for x in ALL if x[0] == name)
        X, x2d, conf = fc.flat(c)
        a, b = kernel(X, x2d, conf, kw), kernel(X, x2d, conf, kw)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)


@pytest.mark.gpu
def test_masked_points_keep_their_X_and_a_group_with_five_points_fails_alone():
    name, c, kw, n_points, masked = fc.masked_case()
    X, x2d, conf = fc.flat(c)
    got = kernel(X, x2d, conf, kw)
    want = fr.refine_cameras_points(X, x2d, conf=conf, **kw)
    assert np.array_equal(got["n_points"], n_points) and np.array_equal(got["n_points"], want["n_points"])
    bad = n_points < rr.MIN_POINTS
    assert bad.sum() == 1 and np.array_equal(got["success"], ~bad)
    for k in INVARIANT_KEYS + GAUGE_KEYS + ("err",):
        _close(got[k], want[k], f"{name}: {k}")
    for k in ("R", "t", "cost0", "cost", "mean_err", "rms_err", "max_err", "moved", "R_rel", "t_rel"):
        assert np.isnan(got[k][bad]).all() and np.isfinite(got[k][~bad]).all(), k
    assert (got["n_evals"][bad] == 0).all() and np.isfinite(got["K"]).all()
    # bitwise: every masked point (NaN X, NaN keypoint, score under min_conf) and the whole failed group keep X
    _, used = rr.weights_and_mask(X, x2d, conf, fc.MIN_CONF)
    used = used & np.repeat(~bad, fc.J)
    assert all(not used[s * fc.J + j] for s, j in masked)
    Xb, Ob = X.view(np.uint64), got["X_opt"].view(np.uint64)
    assert np.array_equal(Ob[~used], Xb[~used])
    assert (got["X_opt"][used] != X[used]).any(axis=1).all()
    assert np.array_equal(~np.isnan(got["err"]), np.stack([used, used]))
    # the neighbours' results are bitwise those of a call without the failed group
    keep = np.repeat(~bad, fc.J)
    rest = kernel(X[keep], x2d[:, keep], conf[:, keep], dict(kw, R0=kw["R0"][~bad], t0=kw["t0"][~bad]))
    for k in got:
        a = got[k][:, keep] if k == "err" else got[k][keep] if k == "X_opt" else got[k][~bad]
        assert np.array_equal(a, rest[k], equal_nan=True), k


@pytest.mark.gpu
def test_absent_start_is_the_resections_dlt_start():
    _, c, kw = next(x for x in ALL if x[0] == "step_V2_lx1")
    X, x2d, conf = fc.flat(c)
    kw = {k: v for k, v in kw.items() if k not in ("R0", "t0")}
    got = kernel(X, x2d, conf, kw)
    start = rr.resect_cameras(X, x2d, K=kw["K"], group_size=fc.J, max_evals=1)
    want = fr.refine_cameras_points(X, x2d, R0=start["R"], t0=start["t"], **kw)
    assert got["success"].all()
    for k in INVARIANT_KEYS + GAUGE_KEYS + ("err",):
        _close(got[k], want[k], k)


@pytest.mark.gpu
def test_solve_rt_and_points_writes_the_references_keys_and_X_opt(tmp_path):
    name, c, kw, n_points, masked = fc.masked_case()
    out = tmp_path / "sub" / "rt_points.npz"
    res = run.solve_rt_and_points(c["X"], c["x2d"][0], c["x2d"][1], conf_left=c["conf"][0], conf_right=c["conf"][1],
                                  K_left=c["K"][0], K_right=c["K"][1], lambda_x=1.0, huber=2.0, min_conf=fc.MIN_CONF, out=out)
    z = np.load(out)
    assert sorted(z.files) == sorted(run.RT_KEYS + ("X_opt", "mask")) == sorted(res)
    X, x2d, conf = fc.flat(c)
    N = X.shape[0]
    assert z["X_opt"].shape == (N, 3) and z["mask"].shape == (N,) and z["mask"].dtype == bool
    assert z["RL"].shape == (3, 3) and z["t_rel"].shape == (3,) and z["mean_err_L"].shape == ()
    assert int(z["n_points"]) == int(n_points.sum()) == int(z["mask"].sum()) and int(z["success"]) == 1
    kw2 = dict(K=c["K"], conf=conf, loss="soft_l1", f_scale=2.0, min_conf=fc.MIN_CONF)
    start = rr.resect_cameras(X, x2d, max_evals=1, **kw2)
    want = fr.refine_cameras_points(X, x2d, R0=start["R"], t0=start["t"], lambda_x=1.0, **kw2)
    _, used = rr.weights_and_mask(X, x2d, conf, fc.MIN_CONF)
    assert np.array_equal(z["mask"], used)
    for key, w in (("RL", want["R"][0, 0]), ("tL", want["t"][0, 0]), ("RR", want["R"][0, 1]), ("tR", want["t"][0, 1]),
                   ("R_rel", want["R_rel"][0, 1]), ("t_rel", want["t_rel"][0, 1]), ("K_L", c["K"][0]), ("K_R", c["K"][1]),
                   ("mean_err_L", want["mean_err"][0, 0]), ("mean_err_R", want["mean_err"][0, 1]),
                   ("median_err_L", np.nanmedian(want["err"][0])), ("median_err_R", np.nanmedian(want["err"][1])),
                   ("X_opt", want["X_opt"])):
        _close(z[key], w, key)
    assert np.array_equal(z["X_opt"].view(np.uint64)[~used], X.view(np.uint64)[~used])
    # (T, J, .) inputs and an absent K, as solve_rt_from_3d takes them; the old entry point still refuses the mode
    one = run.solve_rt_and_points(c["X"], c["x2d"][0], c["x2d"][1], K_left=c["K"][0], lambda_x=100.0)
    _close(one["K_R"], rr.infer_K(x2d[1][np.isfinite(X).all(1) & np.isfinite(x2d).all(axis=(0, 2))]), "inferred K_R")
    assert np.array_equal(one["K_L"], c["K"][0]) and one["X_opt"].shape == (N, 3)
    with pytest.raises(NotImplementedError, match="DESIGN"):
        run.solve_rt_from_3d(X, x2d[0], x2d[1], refine="camera_points")


@pytest.mark.gpu
def test_cpu_tensors_and_bad_shapes_are_rejected():
    c = fc.rig(T=2, V=2, seed=1)
    X, x2d, _ = fc.flat(c)
    with pytest.raises(_lib.SkimiError, match="device tensors"):
        geometry.refine_cameras_points(torch.from_numpy(X), torch.from_numpy(x2d))
    with pytest.raises(ValueError):
        geometry.refine_cameras_points(dev(X), dev(x2d[:, :-1]))
    with pytest.raises(ValueError):
        geometry.refine_cameras_points(dev(X), dev(x2d), loss="huber")
    with pytest.raises(ValueError):
        geometry.refine_cameras_points(dev(X), dev(x2d), R0=dev(np.zeros((1, 2, 3, 3))))
    with pytest.raises(_lib.SkimiError, match="does not divide"):
        geometry.refine_cameras_points(dev(X), dev(x2d), group_size=5)
    with pytest.raises(_lib.SkimiError, match="views"):
        geometry.refine_cameras_points(dev(X), dev(np.concatenate([x2d, x2d, x2d[:1]])))


@pytest.mark.gpu
def test_bad_arguments_return_an_error_code_without_a_launch():
    lib = _lib.lib()
    c = fc.rig(T=2, V=2, seed=1)
    X, x2d, _ = fc.flat(c)
    N = X.shape[0]
    Xd, xd = dev(X), dev(x2d)
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda")    # noqa: E731
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")        # noqa: E731
    R0, t0, Kd = dev(np.stack([c["R"]])), dev(np.stack([c["t"]])), dev(c["K"])
    # R, t, K_out, X_opt, cost0, cost, n_evals, n_used, success, err, stats, moved
    outs = [f64(1, 2, 3, 3), f64(1, 2, 3), f64(1, 2, 3, 3), f64(N, 3), f64(1), f64(1), i32(1), i32(1), i32(1), f64(2, N), f64(1, 2, 3), f64(1)]
    nws = lib.skimi_refine_workspace_bytes(N, 2, N)
    assert nws == (12 + 18 * 2) * N * 8 and lib.skimi_refine_workspace_bytes(N, 5, N) == 0
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

    def call(X=Xd, x2d=xd, R0=R0, t0=t0, n=N, views=2, gs=N, lambda_x=1.0, loss=0, f_scale=1.0, max_evals=200, outs=outs, ws=ws,
             ws_bytes=nws):
        p = [None if o is None else o.data_ptr() for o in outs]
        return lib.skimi_refine_cameras_points(_lib.ptr(X), _lib.ptr(x2d), None, _lib.ptr(Kd), _lib.ptr(R0), _lib.ptr(t0), n, views, gs,
                                               lambda_x, loss, f_scale, 0.0, max_evals, *p, _lib.ptr(ws), ws_bytes, None)

    for kw, msg in ((dict(X=None), b"NULL input"), (dict(x2d=None), b"NULL input"), (dict(R0=None), b"NULL start"),
                    (dict(t0=None), b"NULL start"), (dict(outs=[None] + outs[1:]), b"NULL output"),
                    (dict(outs=outs[:-1] + [None]), b"NULL output"), (dict(views=0), b"views"), (dict(views=5), b"views"),
                    (dict(gs=0), b"does not divide"), (dict(gs=5), b"does not divide"), (dict(n=0), b"does not divide"),
                    (dict(n=800_000_000, gs=800_000_000), b"32-bit point offsets"), (dict(loss=2), b"unknown loss"),
                    (dict(f_scale=0.0), b"f_scale"), (dict(lambda_x=-1.0), b"lambda_x"), (dict(max_evals=0), b"max_evals"),
                    (dict(ws=None), b"workspace"), (dict(ws_bytes=nws - 8), b"workspace"),
                    (dict(outs=outs[:3] + [Xd] + outs[4:]), b"must not be X")):
        assert call(**kw) == -1, kw                      # SKIMI_ERR_ARG
        assert msg in lib.skimi_last_error(), (kw, lib.skimi_last_error())
    torch.cuda.synchronize()
    for o in outs:                                       # nothing was launched: the outputs are untouched
        assert bool((o == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    # K is given: an inferred one (f = 2 std of the keypoints, a fifth of the truth) leaves residuals of tens of pixels,
    # from which kernel and restatement alike use up max_evals (DESIGN, rule 9)
    assert int(outs[7][0]) == N and int(outs[8][0]) == 1 and 1 < int(outs[6][0]) < 200
