"""GPU: the person-origin kernel (csrc/person.hip; geometry.person_origin / recenter_cameras), the triage kernel
(geometry.triangulate_triage) and their use in infer.process_multi_view_clip / process_multi_view_video, against the
float64 restatement of tests/person_restated.py.

Bounds: counts, the median and the keep masks are exact; std, origin, err, depth, view_stats and report within
1e-9 (1 + |x|) (a float64 sum of N <= 268 324 float32 terms in any order is within N 2^-53 ~ 3e-11 relative; 1e-9 is
that with a factor 30, the bound of test_icp_gpu.py).  A kept set (a keep flag) can differ between two correct
implementations only through a point whose | |z - median| - 3 std | (a joint whose |em - threshold|) is at rounding
level, so every case asserts on the restatement, before the kernel runs, that it holds no such point."""
import json

import numpy as np
import pytest
import torch

import person_restated as ref
from skiing_analysis_pytorch_amd import fuse, geometry, infer, vggt, weights as W
from skiing_analysis_pytorch_amd import multi_view_process as mv
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

SOURCE = (1080, 1920)


def _scene(rng, M, H, W, ties=False, negative=False):
    P = rng.normal(0.0, 1.0, (M, H, W, 3)).astype(np.float32)
    z = rng.normal(-1.0 if negative else 5.0, 1.5 if negative else 0.4, (M, H, W))
    bg = rng.random((M, H, W)) < 0.30
    z[bg] = rng.normal(20.0, 3.0, int(bg.sum()))
    if ties:
        z = np.round(z * 4.0) / 4.0          # a few dozen distinct depths: thousands of points share the median
    P[..., 2] = z.astype(np.float32)
    flat = P.reshape(-1)
    flat[rng.random(flat.size) < 0.01] = np.nan
    flat[rng.random(flat.size) < 0.005] = np.inf
    return P


def _boxes(rng, M, src=SOURCE):
    x = np.sort(rng.uniform(0, src[1], (M, 2)), axis=1)
    y = np.sort(rng.uniform(0, src[0], (M, 2)), axis=1)
    return np.stack([x[:, 0], y[:, 0], x[:, 1] + 40, y[:, 1] + 40], axis=1).astype(np.float32)


def person_cases():
    """(name, maps [M, H, W, 3] float32, boxes [M, 4] float32, source (h, w))"""
    rng = np.random.default_rng(2024)
    full = np.array([0, 0, SOURCE[1], SOURCE[0]], np.float32)
    cases = []
    P = _scene(rng, 2, 518, 518)
    cases.append(("518x518 typical boxes, M=2", P, np.array([[700, 300, 1100, 700], [640.5, 250.25, 1000, 811]], np.float32), SOURCE))
    cases.append(("518x518 full frame, M=1", P[:1], full[None], SOURCE))
    cases.append(("294x518 random boxes, M=2", _scene(rng, 2, 294, 518), _boxes(rng, 2), SOURCE))
    cases.append(("41x37 random boxes, M=64", _scene(rng, 64, 41, 37), _boxes(rng, 64), SOURCE))
    edge = np.array([[-300, -200, 600, 500],        # partly outside (top left)
                     [1700, 900, 2500, 1500],       # partly outside (bottom right)
                     [2000, 100, 2300, 900],        # wholly to the right: the reference's clip leaves the last column
                     [100, -900, 900, -10],         # wholly outside in y
                     [900, 300, 500, 700],          # inverted in x
                     [500, 700, 900, 300]], np.float32)
    cases.append(("294x518 boxes outside / inverted, M=6", _scene(rng, 6, 294, 518), edge, SOURCE))
    # 7 x 5 maps, full frame: 35 valid points (odd), 34 (even), 2, 1
    small = rng.normal(3.0, 1.0, (4, 7, 5, 3)).astype(np.float32)
    small[1, 0, 0, 1] = np.nan
    small[2].reshape(-1, 3)[2:] = np.inf
    small[3].reshape(-1, 3)[1:] = np.nan
    cases.append(("7x5 odd / even / two / one valid, M=4", small, np.tile(np.array([0, 0, 5, 7], np.float32), (4, 1)), (7, 5)))
    const = _scene(rng, 2, 64, 48)
    const[0, ..., 2] = 4.25                                       # one repeated depth: std = 0, nothing kept
    const[1] = np.nan                                             # no valid point
    cases.append(("constant depth and all-NaN, M=2", const, np.tile(np.array([0, 0, 48, 64], np.float32), (2, 1)), (64, 48)))
    cases.append(("heavy ties, even and odd counts, M=3", _scene(rng, 3, 120, 90, ties=True),
                  np.array([[0, 0, 90, 120], [0, 0, 89, 120], [3, 5, 80, 111]], np.float32), (120, 90)))
    cases.append(("negative depths, M=2", _scene(rng, 2, 100, 100, negative=True), _boxes(rng, 2, (100, 100)), (100, 100)))
    return cases


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = np.isnan(want) | (got == want) | (np.abs(got - want) <= 1e-9 * (1 + np.abs(want)))
    assert ok.all(), (what, float(np.nanmax(np.abs(got - want))))


@pytest.mark.gpu
@pytest.mark.parametrize("case", person_cases(), ids=lambda c: c[0])
def test_person_origin_matches_restatement(case):
    name, P, boxes, src = case
    want = [ref.person_origin(P[m], boxes[m], src) for m in range(len(P))]
    for m, r in enumerate(want):
        assert ref.margin(r) > 1e-6, (name, m)      # the condition under which the kept sets must be equal
    Pd, bd = torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda()
    got = geometry.person_origin(Pd, bd, src)
    stats = got.stats.cpu().numpy()
    assert stats.shape == (len(P), 8) and got.origin.shape == (len(P), 3) and got.origin.dtype == torch.float64
    for key, col in (("n_box", 0), ("n_valid", 1), ("n_kept", 2)):
        assert stats[:, col].tolist() == [float(r[key]) for r in want], key
    assert got.n_valid.cpu().tolist() == [r["n_valid"] for r in want] and got.n_kept.dtype == torch.int64
    med = np.array([r["median"] for r in want])
    assert np.array_equal(np.isnan(stats[:, 3]), np.isnan(med)) and (np.isnan(med) | (stats[:, 3] == med)).all()
    _close(stats[:, 4], [r["std"] for r in want], "std")
    _close(stats[:, 5:8], np.stack([r["origin"] for r in want]), "origin")
    _close(got.origin.cpu().numpy(), np.stack([r["origin"] for r in want]), "origin")
    # bitwise equal from run to run
    again = geometry.person_origin(Pd, bd, src).stats.cpu().numpy()
    assert np.array_equal(stats.view(np.uint64), again.view(np.uint64))


@pytest.mark.gpu
def test_person_origin_case_properties():
    """what the case list is meant to contain, checked on the kernel's own output"""
    by_name = {c[0]: c for c in person_cases()}
    _, P, boxes, src = by_name["7x5 odd / even / two / one valid, M=4"]
    s = geometry.person_origin(torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda(), src).stats.cpu().numpy()
    assert s[:, 1].tolist() == [35, 34, 2, 1]
    z = np.sort(P[1].reshape(-1, 3)[np.isfinite(P[1].reshape(-1, 3)).all(axis=1), 2].astype(np.float64))
    assert s[1, 3] == (z[16] + z[17]) / 2 and z[16] != z[17]
    assert s[3, 4] == 0 and s[3, 2] == 0 and np.isnan(s[3, 5:]).all()        # one point: std = 0 keeps nothing
    _, P, boxes, src = by_name["constant depth and all-NaN, M=2"]
    s = geometry.person_origin(torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda(), src).stats.cpu().numpy()
    assert s[0, 3] == 4.25 and s[0, 4] == 0 and s[0, 2] == 0 and s[0, 1] > 0 and np.isnan(s[0, 5:]).all()
    assert s[1, 0] == 64 * 48 and s[1, 1] == 0 and np.isnan(s[1, 3:]).all()
    _, P, boxes, src = by_name["294x518 boxes outside / inverted, M=6"]
    s = geometry.person_origin(torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda(), src).stats.cpu().numpy()
    assert (s[:2, 0] > 0).all() and s[3:, 0].tolist() == [0, 0, 0] and np.isnan(s[3:, 3:]).all()
    assert s[2, 0] == ref.crop(boxes[2], (294, 518), src)[3] - ref.crop(boxes[2], (294, 518), src)[1]   # one column wide
    _, P, boxes, src = by_name["heavy ties, even and odd counts, M=3"]
    s = geometry.person_origin(torch.from_numpy(P).cuda(), torch.from_numpy(boxes).cuda(), src).stats.cpu().numpy()
    assert {int(v) % 2 for v in s[:, 1]} == {0, 1} and (s[:, 3] * 8 == np.round(s[:, 3] * 8)).all()
    # batched leading shape [B, S]
    _, P, boxes, src = by_name["518x518 typical boxes, M=2"]
    po = geometry.person_origin(torch.from_numpy(P).cuda()[None], torch.from_numpy(boxes).cuda()[None], src)
    assert po.origin.shape == (1, 2, 3) and po.n_kept.shape == (1, 2) and po.stats.shape == (1, 2, 8)


def _rig(V, J, T, seed, noise=0.7):
    """T steps of V cameras on an arc looking at J points near the origin; keypoints = projections + pixel noise"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    K = np.empty((T, V, 3, 3))
    R = np.empty((T, V, 3, 3))
    t = np.empty((T, V, 3))
    for i in range(T):
        for v in range(V):
            ang = (v - (V - 1) / 2) * 0.25 + rng.normal(scale=0.02)
            R[i, v] = Rotation.from_rotvec([rng.normal(scale=0.02), ang, rng.normal(scale=0.02)]).as_matrix()
            t[i, v] = [rng.normal(scale=0.1), rng.normal(scale=0.1), 6.0 + rng.normal(scale=0.2)]
            K[i, v] = [[600 + 10 * v, 0, 320], [0, 605 + 5 * v, 240], [0, 0, 1]]
    X = rng.normal(size=(T, J, 3)) * [0.5, 0.8, 0.4]
    kp = np.empty((T, V, J, 2))
    for i in range(T):
        for v in range(V):
            p = (X[i] @ R[i, v].T + t[i, v]) @ K[i, v].T
            kp[i, v] = p[:, :2] / p[:, 2:3]
    kp += rng.normal(scale=noise, size=kp.shape) * rng.choice([1.0, 4.0], size=(T, 1, J, 1), p=[0.7, 0.3])
    conf = rng.uniform(0.2, 1.0, (T, V, J))
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()   # noqa: E731
    return f32(K), f32(R), f32(t), f32(kp), f32(conf)


def _check_triage(K, R, t, kp, conf, **kw):
    got = geometry.triangulate_triage(K, R, t, kp, conf, **kw)
    X, X_clean, err, depth, keep, view_stats, report = got
    plain = geometry.triangulate_joints(K, R, t, kp).cpu().numpy()
    Xn = X.cpu().numpy()
    assert np.array_equal(np.isnan(Xn), np.isnan(plain))
    ok = np.isnan(plain) | (np.abs(Xn - plain) <= np.spacing(np.abs(plain)))
    assert ok.all(), "X differs from triangulate_joints by more than one float32 ulp"
    n = lambda a: None if a is None else a.cpu().numpy()   # noqa: E731
    want = ref.triage(n(K), n(R), n(t), n(kp), Xn, n(conf), **kw)
    thr = kw.get("err_thresh_px", 2.0)
    em = want["em"][np.isfinite(want["em"])]
    assert np.abs(em - thr).min() > 1e-6                   # no joint at the threshold: the keep masks must be equal
    _close(err.cpu().numpy(), want["err"], "err")
    _close(depth.cpu().numpy(), want["depth"], "depth")
    _close(view_stats.cpu().numpy(), want["view_stats"], "view_stats")
    _close(report.cpu().numpy(), want["report"], "report")
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want["keep"])
    Xc = X_clean.cpu().numpy()
    assert np.array_equal(np.isnan(Xc).all(axis=-1), ~want["keep"]) and np.array_equal(Xc[want["keep"]], Xn[want["keep"]])
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("V,J", [(2, 17), (3, 12), (8, 17), (2, 12)])
def test_triangulate_triage_matches_restatement(V, J):
    K, R, t, kp, conf = _rig(V, J, T=4, seed=10 * V + J)
    got, want = _check_triage(K, R, t, kp, conf)
    assert 0 < want["keep"].sum() < want["keep"].size          # the case exercises both verdicts
    got2, want2 = _check_triage(K, R, t, kp, None)
    assert want2["keep"].sum() > want["keep"].sum()            # ... and the scores reject some joints on their own
    _check_triage(K, R, t, kp, conf, conf_thr=0.5, err_thresh_px=1.0)
    again = geometry.triangulate_triage(K, R, t, kp, conf)
    for a, b in zip(got, again):
        assert torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0))


@pytest.mark.gpu
def test_triangulate_triage_nan_keypoint_and_behind_camera():
    K, R, t, kp, conf = _rig(2, 17, T=3, seed=5)
    kp[1, 0, 4, 0] = float("nan")
    # step 2: view 1 looks the other way -- every joint is behind it
    R[2, 1] = torch.diag(torch.tensor([-1.0, 1.0, -1.0], device="cuda")) @ R[2, 1]
    t[2, 1] = torch.tensor([-1.0, 1.0, -1.0], device="cuda") * t[2, 1]
    got, want = _check_triage(K, R, t, kp, conf)
    assert torch.isnan(got.err[1, :, 4]).all() and not bool(got.keep[1, 4]) and torch.isfinite(got.view_stats).all()
    assert torch.isnan(got.X[1, 4]).all()
    behind = (got.depth[2] <= 0).any(dim=0)          # noisy keypoints: the DLT puts some joints in front of it again
    assert behind.any() and not got.keep[2][behind].any()
    assert float(got.report[2, 2]) == float((~behind).double().mean())


@pytest.mark.gpu
def test_recenter_cameras_matches_restatement():
    rng = np.random.default_rng(8)
    from scipy.spatial.transform import Rotation
    for S in (2, 3):
        n = 5
        E = np.concatenate([Rotation.from_rotvec(rng.normal(scale=0.4, size=(n * S, 3))).as_matrix().reshape(n, S, 3, 3),
                            rng.normal(size=(n, S, 3, 1))], axis=-1).astype(np.float32)
        stats = np.zeros((n, S, 8))
        stats[..., 2] = rng.integers(1, 100, (n, S))
        stats[..., 5:] = rng.normal(size=(n, S, 3)) * 3
        stats[1, 0, 2] = 0                      # a view that kept nothing: origin zero
        stats[1, 0, 5:] = np.nan
        origin, R, t = geometry.recenter_cameras(torch.from_numpy(stats).cuda(), torch.from_numpy(E).cuda())
        for i in range(n):
            o, Rw, tw = ref.recenter(stats[i, :, 5:], stats[i, :, 2], E[i, :, :, :3], E[i, :, :, 3])
            _close(origin[i].cpu().numpy(), o, "origin")
            assert np.array_equal(R[i].cpu().numpy(), Rw.astype(np.float32))
            tg = t[i].cpu().numpy()
            assert (np.abs(tg - tw) <= np.spacing(np.abs(tw).astype(np.float32))).all()
        assert not origin[1].any()


# ---- the clip path with the tiny model ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    return m


def _clip_inputs(T=5, S=2, H=140, Wd=140):
    frames = torch.stack([W.make_images(S, H, Wd, seed=80 + t) for t in range(T)])
    g = torch.Generator().manual_seed(11)
    kps = torch.rand((T, S, 17, 2), generator=g) * (Wd - 40) + 20
    boxes = torch.tensor([[30.0, 20, 110, 120], [25.5, 30, 120, 131], [10.25, 5, 100, 90]]).repeat(T, 1, 1)[:, :S]
    boxes = boxes + torch.rand((T, S, 4), generator=g) * 4
    scores = torch.rand((T, S, 17), generator=g) * 0.8 + 0.2
    return frames, kps, boxes, scores


@pytest.mark.gpu
def test_clip_without_the_new_arguments_is_the_chain_of_public_functions(tiny):
    """process_multi_view_clip without boxes / scores / triage = model call -> pose_encoding_to_extri_intri ->
    triangulate_joints per chunk of steps, bit for bit (the fp32-accurate mode is run-to-run deterministic)"""
    frames, kps, _, _ = _clip_inputs(S=3)
    frames, kps = frames.cuda(), kps.cuda()
    out = infer.process_multi_view_clip(tiny, frames, kps, steps_per_call=2)
    assert sorted(out) == ["extrinsic", "intrinsic", "joints3d"]
    J, Es, Ks = [], [], []
    for a in range(0, 5, 2):
        idx = list(range(a, min(a + 2, 5)))
        pe = tiny(frames[idx], want={"camera"})["pose_enc"]
        E, K = geometry.pose_encoding_to_extri_intri(pe, (140, 140))
        J.append(geometry.triangulate_joints(K, E[..., :3, :3].contiguous(), E[..., :3, 3].contiguous(), kps[idx]))
        Es.append(E)
        Ks.append(K)
    assert torch.equal(out["joints3d"], torch.cat(J)) and torch.equal(out["extrinsic"], torch.cat(Es))
    assert torch.equal(out["intrinsic"], torch.cat(Ks))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 3])
def test_clip_with_boxes_and_triage_matches_restated_chain(tiny, S):
    frames, kps, boxes, scores = _clip_inputs(S=S)
    T, H, Wd = 5, 140, 140
    fd, kd = frames.cuda(), kps.cuda()
    out = infer.process_multi_view_clip(tiny, fd, kd, steps_per_call=2, smooth=True, boxes=boxes.cuda(), scores=scores.cuda(),
                                        triage=True, err_thresh_px=40.0)
    want_keys = {"joints3d", "extrinsic", "intrinsic", "origin", "R", "t", "joints3d_clean", "reproj_err", "keep", "view_stats",
                 "triage_report", "joints3d_smoothed", "joints3d_clean_smoothed"}
    assert set(out) == want_keys
    assert out["origin"].dtype == torch.float64 and out["keep"].dtype == torch.bool and out["reproj_err"].shape == (T, S, 17)
    # the model's own depth and cameras, chunked as the call chunks them
    for a in range(0, T, 2):
        idx = list(range(a, min(a + 2, T)))
        o = tiny(fd[idx], want={"camera", "depth"})
        E, K = geometry.pose_encoding_to_extri_intri(o["pose_enc"], (H, Wd))
        assert torch.equal(E, out["extrinsic"][idx]) and torch.equal(K, out["intrinsic"][idx])
        for b, i in enumerate(idx):
            wp = geometry.unproject_depth_map_to_point_map(o["depth"][b], E[b], K[b]).cpu().numpy()
            for v in range(S):
                assert ref.margin(ref.person_origin(wp[v], boxes[i, v].numpy(), (H, Wd))) > 1e-6
            Rg, tg = out["R"][i].cpu().numpy(), out["t"][i].cpu().numpy()
            r = ref.step_chain(wp, boxes[i].numpy(), (H, Wd), E[b].cpu().numpy(), K[b].cpu().numpy(), kps[i].numpy(),
                               out["joints3d"][i].cpu().numpy(), scores[i].numpy(), err_thresh_px=40.0, cameras=(Rg, tg))
            _close(out["origin"][i].cpu().numpy(), r["origin"], "origin")
            assert np.array_equal(Rg, r["R"])
            assert (np.abs(tg - r["t"]) <= np.spacing(np.abs(r["t"]))).all()
            tri = r["triage"]
            em = tri["em"][np.isfinite(tri["em"])]
            assert np.abs(em - 40.0).min() > 1e-6
            _close(out["reproj_err"][i].cpu().numpy(), tri["err"][0], "reproj_err")
            _close(out["view_stats"][i].cpu().numpy(), tri["view_stats"][0], "view_stats")
            _close(out["triage_report"][i].cpu().numpy(), tri["report"][0], "report")
            assert np.array_equal(out["keep"][i].cpu().numpy(), tri["keep"][0])
            # the joints are the plain DLT through the recentred cameras
            X = geometry.triangulate_joints(K[b:b + 1], out["R"][i:i + 1], out["t"][i:i + 1], kd[i:i + 1])[0]
            assert torch.equal(X.nan_to_num(nan=-7.0), out["joints3d"][i].nan_to_num(nan=-7.0))
    if S == 2:   # the turn of view 1
        assert torch.equal(out["R"][:, 1, 0], -out["extrinsic"][:, 1, 0, :3]) and torch.equal(out["R"][:, 1, 1], out["extrinsic"][:, 1, 1, :3])
    else:
        assert torch.equal(out["R"], out["extrinsic"][..., :3])
    clean = out["joints3d_clean"].cpu().numpy().astype(np.float64)
    assert np.array_equal(out["joints3d_clean_smoothed"].numpy(), fuse.smooth_skeleton(clean), equal_nan=True)
    # boxes without triage: the same cameras and joints, no verdict
    ob = infer.process_multi_view_clip(tiny, fd, kd, steps_per_call=2, boxes=boxes.cuda())
    assert set(ob) == {"joints3d", "extrinsic", "intrinsic", "origin", "R", "t"}
    assert torch.equal(ob["t"], out["t"]) and torch.equal(ob["origin"], out["origin"])
    assert torch.equal(ob["joints3d"].nan_to_num(nan=-7.0), out["joints3d"].nan_to_num(nan=-7.0))
    # two batches in flight give the same clip
    o2 = infer.process_multi_view_clip(tiny, fd, kd, steps_per_call=1, streams=2, boxes=boxes.cuda(), scores=scores.cuda(),
                                       triage=True, err_thresh_px=40.0)
    assert np.abs((o2["origin"] - out["origin"]).cpu().numpy()).max() < 1e-4
    assert o2["keep"].shape == out["keep"].shape


@pytest.mark.gpu
def test_clip_does_not_wait_on_the_device_between_model_call_and_gather(tiny, monkeypatch):
    """With everything on, between the return of the model call and the all-gather torch sees no synchronising
    operation (no device -> host copy, no host wait): its sync debug mode is set to "error" for exactly that span.  One
    call of six steps on a shard padded from T = 5 to 6, so the repeat of the last step is covered.  What this can see:
    torch's own synchronising calls (a .cpu(), .item(), a list index's upload -- which is what the first version of
    this path did and this test caught).  What it cannot see: a hipStreamSynchronize inside libskimi (the three new
    launches, skimi_person_origin, skimi_recenter_cameras and skimi_triangulate_triage, contain none: csrc/person.hip,
    csrc/geometry.hip), and streams > 1, whose worker threads it does not cover."""
    from skiing_analysis_pytorch_amd import parallel
    frames, kps, boxes, scores = (a.cuda() for a in _clip_inputs())
    infer.process_multi_view_clip(tiny, frames, kps, steps_per_call=6, boxes=boxes, scores=scores, triage=True)   # sizes the workspaces
    spans = []

    def model(*a, **k):
        torch.cuda.set_sync_debug_mode("default")
        out = tiny(*a, **k)
        torch.cuda.set_sync_debug_mode("error")
        spans.append(1)
        return out

    real_gather = parallel.all_gather_packed

    def gather(parts, T):
        torch.cuda.set_sync_debug_mode("default")
        return real_gather(parts, T)

    monkeypatch.setattr(parallel, "all_gather_packed", gather)
    monkeypatch.setattr(parallel, "shard_range", lambda T: (0, 6, 6))
    try:
        out = infer.process_multi_view_clip(model, frames, kps, steps_per_call=6, boxes=boxes, scores=scores, triage=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(spans) == 1 and out["keep"].shape == (5, 17) and out["origin"].shape == (5, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("with_boxes", [True, False])
def test_clip_chunk_wholly_in_the_padding(tiny, monkeypatch, with_boxes):
    """A rank whose block, or whose last chunk, starts beyond the clip (T = 5 on a shard padded to 8: T = 5 on 4 ranks
    gives rank 3 the steps 6, 7) computes the last step again for every padded step: as many rows as steps, each equal to
    what a single process computes for step 4.  With boxes and without (triage alone takes its step count from the
    keypoints)."""
    from skiing_analysis_pytorch_amd import parallel
    frames, kps, boxes, scores = (a.cuda() for a in _clip_inputs())
    kw = dict(scores=scores, triage=True, err_thresh_px=40.0, **({"boxes": boxes} if with_boxes else {}))
    one = infer.process_multi_view_clip(tiny, frames, kps, steps_per_call=1, **kw)
    seen = []
    real = parallel.all_gather_packed
    monkeypatch.setattr(parallel, "all_gather_packed", lambda parts, T: (seen.append([p.shape[0] for p in parts]), real(parts, T))[1])
    # one step per call: chunks (6, 7) and (7, 8), the same model calls as the single process makes for step 4
    monkeypatch.setattr(parallel, "shard_range", lambda T: (6, 8, 8))
    pad = infer.process_multi_view_clip(tiny, frames, kps, steps_per_call=1, **kw)
    assert set(seen[-1]) == {2} and set(pad) == set(one)
    for k, v in one.items():
        for row in pad[k]:
            assert torch.equal(row.nan_to_num(nan=-7.0), v[4].nan_to_num(nan=-7.0)), k
    # chunks (4, 6) -- half inside -- and (6, 8) -- wholly beyond -- in calls of two steps
    monkeypatch.setattr(parallel, "shard_range", lambda T: (4, 8, 8))
    pad2 = infer.process_multi_view_clip(tiny, frames, kps, steps_per_call=2, **kw)
    assert set(seen[-1]) == {4}
    for k, v in one.items():
        assert pad2[k].shape == (4, *v.shape[1:]), k
    assert torch.equal(pad2["keep"], one["keep"][4].expand(4, -1))
    assert ((pad2["joints3d"] - one["joints3d"][4]).abs().nan_to_num() / (1 + one["joints3d"][4].abs().nan_to_num())).max() < 1e-4


def _rank_worker(rank, world, port, golden_path, q):
    """one rank of the two-rank clip (gloo; both ranks on cuda:0) with everything switched on, counting the collectives"""
    import os

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = np.load(golden_path)
        cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
        m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
        m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
        frames, kps, boxes, scores = _clip_inputs()
        calls = []
        real = dist.all_gather_into_tensor
        others = {name: getattr(dist, name) for name in ("all_gather", "all_reduce", "broadcast", "all_gather_object")}

        def counting(*a, **k):
            calls.append("all_gather_into_tensor")
            return real(*a, **k)

        dist.all_gather_into_tensor = counting
        for name, fn in others.items():
            setattr(dist, name, lambda *a, _n=name, _f=fn, **k: (calls.append(_n), _f(*a, **k))[1])
        out = infer.process_multi_view_clip(m, frames.cuda(), kps.cuda(), steps_per_call=1, smooth=True, boxes=boxes.cuda(),
                                            scores=scores.cuda(), triage=True, err_thresh_px=40.0)
        q.put((rank, calls, {k: v.cpu().numpy() for k, v in out.items()}))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_clip_with_everything_on_uses_one_all_gather(tiny, golden_dir):
    """T = 5 sharded 3 + 2 over two ranks: exactly one all_gather_into_tensor (and no other collective) moves joints,
    cameras, origin and the triage outputs, and every rank holds what one process computes alone, bit for bit.  One
    time step per model call in both runs, so that both make the same calls: the origin is read off the dense depth
    maps, and those are only reproducible to the last bit between calls of one batch composition."""
    import socket

    import torch.multiprocessing as mp
    frames, kps, boxes, scores = _clip_inputs()
    one = infer.process_multi_view_clip(tiny, frames.cuda(), kps.cuda(), steps_per_call=1, smooth=True, boxes=boxes.cuda(),
                                        scores=scores.cuda(), triage=True, err_thresh_px=40.0)
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(golden_dir / "vggt_tiny_conv.npz"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, calls, out in res:
        assert calls == ["all_gather_into_tensor"], (rank, calls)
        assert set(out) == set(one)
        for k, v in one.items():
            assert out[k].shape == tuple(v.shape) and out[k].dtype == v.cpu().numpy().dtype, k
            assert np.array_equal(out[k], v.cpu().numpy(), equal_nan=True), (rank, k)


def _clip_pt(path, name, frames, kps, boxes, scores):
    T, H, Wd = frames.shape[:3]
    torch.save({"video_name": name, "video_path": f"/videos/{name}.mp4", "frame_count": T, "img_shape": (H, Wd), "fps": 30,
                "detectron2": {"bbox": torch.from_numpy(boxes), "keypoints": torch.from_numpy(kps),
                               "keypoints_score": torch.from_numpy(scores)},
                "depth": torch.zeros(T, 1, 4, 4), "frames": frames}, path)


@pytest.mark.gpu
def test_process_multi_view_video_flags(tiny, tmp_path):
    rng = np.random.default_rng(1)
    T, H, Wd = 5, 135, 240
    lf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    rf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    lk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    rk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    lb = np.tile(np.array([[60, 30, 180, 110]], np.float32), (T, 1))
    rb = np.tile(np.array([[50, 20, 170, 120]], np.float32), (T, 1))
    sc = (rng.random((T, 17)) * 0.8 + 0.2).astype(np.float32)
    (tmp_path / "subj01").mkdir()
    _clip_pt(tmp_path / "subj01" / "left.pt", "left", lf, lk, lb, sc)
    _clip_pt(tmp_path / "subj01" / "right.pt", "right", rf, rk, rb, sc[::-1].copy())
    head = infer.CameraHead({"infer": {"gpu": 0}}, None, model=tiny)

    def run(tag, cfg):
        out_dir = mv.process_multi_view_video(tmp_path / "subj01" / "left.mp4", tmp_path / "subj01" / "left.pt",
                                              tmp_path / "subj01" / "right.mp4", tmp_path / "subj01" / "right.pt",
                                              tmp_path / tag, tmp_path / tag / "inference", cfg, camera_head=head, steps_per_call=2)
        return out_dir, dict(np.load(tmp_path / tag / "inference" / "subj01_multi_view_3d_info.npz"))

    today = {"camera_intrinsics", "R", "t", "C", "x3d", "icp_refined", "x3d_smoothed"}
    d_absent, absent = run("absent", {"infer": {"gpu": 0}})
    d_false, false = run("false", {"infer": {"gpu": 0, "device_origin": False, "triage": False}})
    assert set(absent) == today and set(false) == today
    for k in today:
        assert np.array_equal(absent[k], false[k], equal_nan=True), k
    assert not (d_absent / "raw_reprojection_error.txt").exists()
    d_on, on = run("on", {"infer": {"gpu": 0, "device_origin": True, "triage": True},
                          "triangulation": {"conf_thr": 0.4, "err_thresh_px": 30.0}})
    new = {"reproj_err", "x3d_clean", "triage_keep", "triage_report", "reproj_view_stats"}
    assert set(on) == today | new
    assert on["reproj_err"].shape == (T, 2, 17) and on["triage_keep"].shape == (T, 17) and on["triage_keep"].dtype == bool
    assert on["triage_report"].shape == (T, 5) and on["reproj_view_stats"].shape == (T, 2, 4) and on["x3d_clean"].shape == (T, 17, 3)
    # the device origin is the host path's up to its float32 sums; the cameras and C agree accordingly
    for k in ("R", "C", "camera_intrinsics"):
        assert np.array_equal(on[k], absent[k]), k
    assert np.abs(on["t"] - absent["t"]).max() / (np.abs(absent["t"]).max() + 1) < 1e-4
    # the verdicts are the restatement's on the stored cameras (rounded to float32 as they feed the kernel)
    conf = np.stack([sc, sc[::-1]], axis=1)
    want = ref.triage(on["camera_intrinsics"].astype(np.float32), on["R"].astype(np.float32), on["t"].astype(np.float32),
                      np.stack([lk, rk], axis=1), on["x3d"], conf, 0.4, 30.0)
    _close(on["reproj_err"], want["err"], "reproj_err")
    _close(on["reproj_view_stats"], want["view_stats"], "view_stats")
    assert np.abs(want["em"][np.isfinite(want["em"])] - 30.0).min() > 1e-6 and np.array_equal(on["triage_keep"], want["keep"])
    assert np.array_equal(np.isnan(on["x3d_clean"]).all(axis=-1), ~want["keep"])
    # raw_reprojection_error.txt in the reference's layout
    lines = (d_on / "raw_reprojection_error.txt").read_text().splitlines()
    assert len(lines) == T * 9 and lines[0] == "Frame 0000 Reprojection Error (in pixels):"
    assert [ln.split(":")[0].strip() for ln in lines[1:9]] == ["rmse_L", "rmse_R", "mean_err_L", "mean_err_R", "median_err_L",
                                                               "median_err_R", "max_err_L", "max_err_R"]
    assert float(lines[9 * 3 + 2].split(":")[1]) == on["reproj_view_stats"][3, 1, 0]
    # dense_to_host=False: the slot is None and the device copy stays
    recs = head.reconstruct_batch([0], [[lf[0], rf[0]]], dense_to_host=False)
    assert recs[0][5] is None and head.last_world_points.shape == (1, 2, 294, 518, 3)
