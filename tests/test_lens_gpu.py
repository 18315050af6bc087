"""GPU: the lens kernels (csrc/lens.hip: skimi_distort_points, skimi_undistort_points, skimi_project_points,
skimi_undistort_u8) against the float64 restatement (tests/lens_restated.py, itself held against the reference by
tests/test_lens_cpu.py) on the cases of tests/lens_cases.py.  Points: every float within 1e-9 (1 + |x|), the project's float64
tolerance, for every coefficient count, two cameras with different coefficients in one call, n = 1, 63, 65 and 17 * 243 (one
lane, either side of a wave, many blocks), pixels / normalised / P != K; NaN rows stay in their row; two runs are the same
bits; a camera alone is the same bits as inside the batch.  Frames: equal to the restatement everywhere except at near-tie
pixels (unrounded value within 1e-6 of k + 0.5), which may differ by 1 and are at most 1e-4 of the frame; the input is left
alone and a guard region behind the output is untouched.  Then the distorted two-camera rig through triangulate_triage and
triangulate_robust with dist=, and the entry points with cfg.infer.undistort on the tiny model."""
import json
import logging

import numpy as np
import pytest
import torch

import lens_cases as lc
import lens_restated as lr
from skiing_analysis_pytorch_amd import _lib, calibration, geometry, infer, preprocess, vggt, weights as W
from skiing_analysis_pytorch_amd import multi_view_process as mv
from skiing_analysis_pytorch_amd import single_view_process as sv
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu
TOL = 1e-9


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def close(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ"
    err = np.nanmax(np.abs(got - want) / (1 + np.abs(want))) if want.size else 0.0
    print(f"{what}: max scaled error {err:.3g}")
    assert err <= TOL, what


def restated_undistort(x, K, dist, P=None, **kw):
    r = [lr.undistort_points(x[c], K[c], dist[c], None if P is None else P[c], **kw) for c in range(len(K))]
    return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


@pytest.mark.parametrize("n", lc.POINT_COUNTS)
@pytest.mark.parametrize("k", lr.COEFF_COUNTS)
def test_points_match_restatement(k, n):
    x, K, dist, P = lc.point_case(k, n)
    xd = dev(x)
    for kw in ({}, {"P": P}, {"normalized": True}, {"iters": 5}):
        got = geometry.undistort_points(xd, K, dist, **kw)
        want_x, want_r = restated_undistort(x, K, dist, **kw)
        close(got.x, want_x, f"undistort {kw} k={k} n={n}")
        close(got.resid_px, want_r, f"resid_px {kw} k={k} n={n}")
        again = geometry.undistort_points(xd, K, dist, **kw)
        assert host(again.x).tobytes() == host(got.x).tobytes() and host(again.resid_px).tobytes() == host(got.resid_px).tobytes()
    und = geometry.undistort_points(xd, K, dist, normalized=True).x
    for kw, src in (({}, xd), ({"P": P}, xd), ({"normalized": True}, und)):
        want = np.stack([lr.distort_points(host(src)[c], K[c], dist[c], kw.get("P", [None, None])[c] if "P" in kw else None,
                                           normalized=kw.get("normalized", False)) for c in range(2)])
        close(geometry.distort_points(src, K, dist, **kw), want, f"distort {kw} k={k} n={n}")
    # the inverse really inverts: inside the frame the round trip closes and resid_px says so
    r = geometry.undistort_points(xd, K, dist)
    back = host(geometry.distort_points(r.x, K, dist))
    assert np.abs(back - x).max() < 1e-6 and host(r.resid_px).max() < 1e-6
    # a camera alone is the same bits as the same camera inside the batch
    for c in range(2):
        alone = geometry.undistort_points(xd[c], K[c], dist[c], P=P[c])
        both = geometry.undistort_points(xd, K, dist, P=P)
        assert host(alone.x).tobytes() == host(both.x[c]).tobytes() and host(alone.resid_px).tobytes() == host(both.resid_px[c]).tobytes()


def test_nan_rows_stay_in_their_row():
    x, K, dist, P = lc.point_case(12, 65)
    bad = x.copy()
    bad[0, 7, 0] = np.nan
    bad[1, 64] = np.inf
    bad[1, 0, 1] = np.nan
    ref = geometry.undistort_points(dev(x), K, dist)
    got = geometry.undistort_points(dev(bad), K, dist)
    gx, gr, rx, rr = host(got.x), host(got.resid_px), host(ref.x), host(ref.resid_px)
    rows = [(0, 7), (1, 64), (1, 0)]
    for c, j in rows:
        assert np.isnan(gx[c, j]).all() and np.isnan(gr[c, j])
        rx[c, j] = gx[c, j]
        rr[c, j] = gr[c, j]
    assert gx.tobytes() == rx.tobytes() and gr.tobytes() == rr.tobytes()
    d = host(geometry.distort_points(dev(bad), K, dist))
    assert np.isnan(d[0, 7, 0]) and np.isfinite(d[0, :7]).all() and np.isfinite(d[0, 8:]).all()


def test_fold_over_point_is_exposed():
    K = lc.small_K(1920, 1080, 0.58)
    x = np.array([lc.FOLD_POINT_NORMALIZED, (0.3, 0.2)]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    r = host(geometry.undistort_points(dev(x), K, lc.REF_P4[0]).resid_px)
    print("resid_px beyond the fold-over and inside:", r)
    assert (np.isnan(r[0]) or r[0] > 1.0) and r[1] < 1e-9


def test_batch_shapes_steps_and_identity():
    rig = lc.rig_case()
    kp, K, d = rig["kp"], rig["K"][0], rig["dist"]            # [T, V, J, 2], one calibration per view: one launch
    dist = np.stack([d, np.r_[lc.OTHER, 0, 0]])
    got = geometry.undistort_points(dev(kp), K, dist)
    want = [restated_undistort(kp[i], K, dist) for i in range(kp.shape[0])]
    close(got.x, np.stack([w[0] for w in want]), "undistort [T, V, J, 2]")
    close(got.resid_px, np.stack([w[1] for w in want]), "resid_px [T, V, J]")
    # one K for everything: any leading shape
    one = geometry.undistort_points(dev(kp), K[0], d)
    close(one.x, lr.undistort_points(kp, K[0], d)[0], "undistort [..., 2] with one K")
    # K per (step, view) on the device: the triangulations' path
    Ks = rig["K"] * np.linspace(0.9, 1.1, 4).reshape(2, 2, 1, 1)
    Ks[..., 2, 2] = 1
    steps = geometry.undistort_keypoints_steps(dev(kp), dev(Ks), dist)
    want = np.stack([restated_undistort(kp[i], Ks[i], dist)[0] for i in range(2)])
    close(steps.x, want, "undistort_keypoints_steps")
    # calibration without distortion is no calibration: the same object comes back
    x = dev(kp)
    for zero in (np.zeros(4), np.zeros((2, 14))):
        assert geometry.undistort_points(x, K, zero).x is x and geometry.distort_points(x, K, zero, P=K) is x
    assert float(geometry.undistort_points(x, K, np.zeros(5)).resid_px.abs().max()) == 0.0
    assert geometry.undistort_points(x, K, np.zeros(4), P=K * 0.5).x is not x
    f32 = dev(kp.astype(np.float32))
    assert geometry._undistorted_f32(f32, dev(rig["K"]), np.zeros(14)) is f32
    # empty
    e = geometry.undistort_points(torch.empty((0, 2), dtype=torch.float64, device="cuda"), K[0], d)
    assert e.x.shape == (0, 2) and e.resid_px.shape == (0,)


def test_project_points_matches_restatement():
    rig = lc.rig_case()
    X, R, t, K, d = rig["X"], rig["R"][0], rig["t"][0], rig["K"][0], rig["dist"]
    Xv = np.ascontiguousarray(np.broadcast_to(X[:, None], (2, 2, 25, 3)))              # [T, V, J, 3]
    dist = np.stack([d, np.r_[lc.OTHER, 0, 0]])
    got = geometry.project_points(dev(Xv), R, t, K, dist)
    want = [[lr.project_points(X[i], R[v], t[v], K[v], dist[v]) for v in range(2)] for i in range(2)]
    close(got.x, np.array([[w[0] for w in row] for row in want]), "project_points pixels")
    close(got.depth, np.array([[w[1] for w in row] for row in want]), "project_points depth")
    close(got.x[:, 0], rig["kp"][:, 0], "the rig's keypoints")
    pin = geometry.project_points(dev(X[0]), R[1], t[1], K[1])
    close(pin.x, lr.project_points(X[0], R[1], t[1], K[1])[0], "project_points without coefficients")
    close(pin.x, rig["kp_ideal"][0, 1], "the rig's ideal keypoints")


def test_argument_errors():
    x, K, dist, P = lc.point_case(4, 3)
    with pytest.raises(ValueError, match="tilt"):
        geometry.undistort_points(dev(x), K, [0.1] * 12 + [0.01, 0.0])
    with pytest.raises(ValueError):
        geometry.undistort_points(dev(x), K, [0.1] * 7)
    with pytest.raises(ValueError, match="cameras"):
        geometry.undistort_points(dev(np.zeros((9, 2, 2))), np.tile(K[0], (9, 1, 1)), dist[0])
    with pytest.raises(ValueError):
        geometry.undistort_points(dev(x[:, :, :1]), K, dist)
    with pytest.raises(ValueError):
        geometry.undistort_points(dev(x), K * 0, dist)
    with pytest.raises(_lib.SkimiError):
        geometry.undistort_points(torch.from_numpy(x), K, dist)
    with pytest.raises(_lib.SkimiError):
        preprocess.undistort_images(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), K[0], dist[0])
    with pytest.raises(ValueError):
        preprocess.undistort_images(torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device="cuda"), K[0], dist[0])
    # the library refuses what the wrapper would not let through
    lib = _lib.lib()
    z = torch.zeros(8, dtype=torch.float64, device="cuda")
    Kh = np.ascontiguousarray(K[0])
    assert lib.skimi_undistort_points(z.data_ptr(), Kh.ctypes.data, None, None, None, 1, 9, 1, 5, 0, z.data_ptr(), z.data_ptr(), None) != 0
    assert b"cameras" in lib.skimi_last_error()
    assert lib.skimi_undistort_points(z.data_ptr(), Kh.ctypes.data, None, None, None, 1, 1, 1, -1, 0, z.data_ptr(), z.data_ptr(), None) != 0
    assert lib.skimi_undistort_u8(z.data_ptr(), z.data_ptr(), Kh.ctypes.data, None, None, 1, 1, 2, 2, 2, 2, 2, None) != 0
    assert b"channels" in lib.skimi_last_error()


@pytest.mark.parametrize("name", list(lc.image_cases()))
def test_frames_match_restatement(name):
    case = lc.image_cases()[name]
    imgs = lc.images_of(case)
    want, tie = lc.restated_frames(case, imgs)
    src = dev(imgs)
    keep = src.clone()
    n = want.size
    guard = 4096
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[:n].view(want.shape)
    got = preprocess.undistort_images(src, case["K"], case["dist"], case["new_K"], case["out_size"], out=out)
    assert got is out
    g = host(got)
    assert torch.equal(src, keep), "the input was written"
    assert bool((buf[n:] == 0xA5).all()), "the guard region behind the output was written"
    diff = g.astype(np.int16) - want.astype(np.int16)
    off = diff != 0
    print(f"{name}: {off.sum()} of {n} values differ, near-tie share {tie.mean():.3g}, border share {(want == 0).mean():.3g}")
    assert not (off & ~tie).any(), "a value away from a rounding tie differs"
    assert np.abs(diff).max() <= 1 and tie.mean() <= 1e-4
    # a fresh allocation, one camera alone (four axes), and a second run: the same bytes
    again = preprocess.undistort_images(src, case["K"], case["dist"], case["new_K"], case["out_size"])
    assert host(again).tobytes() == g.tobytes()
    new1 = None if case["new_K"] is None else case["new_K"][1]
    alone = preprocess.undistort_images(src[1], case["K"][1], case["dist"][1], new1, case["out_size"])
    assert alone.shape == want.shape[1:] and host(alone).tobytes() == g[1].tobytes()


def test_frames_unaligned_rows_four_channels_and_identity():
    """W * ch no multiple of 4 (byte stores), ch = 4 and an output whose base is not dword-aligned; zero coefficients with
    new_K = K give the input back, an integer principal-point shift translates it with a zero border"""
    case = lc.image_cases()["37x53"]
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 37, 53, 4), dtype=np.uint8)
    K = case["K"][0]
    same = preprocess.undistort_images(dev(img), K, np.zeros(4))
    assert np.array_equal(host(same), img)
    newK = K.copy()
    newK[0, 2] += 5
    newK[1, 2] -= 3
    want = np.zeros_like(img)
    want[:, :-3, 5:] = img[:, 3:, :-5]
    assert np.array_equal(host(preprocess.undistort_images(dev(img), K, np.zeros(5), newK)), want)
    d = case["dist"][0]
    want = np.stack([lr.undistort_image(img[f], K, d, newK, (47, 31)) for f in range(2)])
    buf = torch.zeros(want.size + 8, dtype=torch.uint8, device="cuda")
    out = buf[1:1 + want.size].view(want.shape)                  # odd base address
    got = host(preprocess.undistort_images(dev(img), K, d, newK, (47, 31), out=out))
    assert np.abs(got.astype(np.int16) - want).max() <= 1 and (got != want).mean() <= 1e-4
    assert int(buf[0]) == 0 and int(buf[1 + want.size:].sum()) == 0


def test_distorted_rig_needs_dist():
    rig = lc.rig_case()
    K, R, t = (dev(rig[k].astype(np.float32)) for k in ("K", "R", "t"))
    kp = dev(rig["kp"].astype(np.float32))
    raw = geometry.triangulate_triage(K, R, t, kp, err_thresh_px=2.0)
    assert int((~raw.keep).sum()) >= 1, "the lens alone must cost joints at 2 px"
    fixed = geometry.triangulate_triage(K, R, t, kp, err_thresh_px=2.0, dist=rig["dist"])
    err = np.abs(host(fixed.X).astype(np.float64) - rig["X"]).max()
    print(f"dropped without dist: {int((~raw.keep).sum())} of {raw.keep.numel()}; with dist max |X - truth| {err:.3g}, "
          f"max reprojection error {float(fixed.err.max()):.3g} px")
    assert bool(fixed.keep.all()) and err < 1e-6
    # triangulate_robust takes the same argument: the call on keypoints undistorted beforehand, bit for bit
    rob = geometry.triangulate_robust(K, R, t, kp, inlier_px=2.0, dist=np.stack([rig["dist"], rig["dist"]]))
    kpu = geometry.undistort_keypoints_steps(kp, K, rig["dist"]).x.to(torch.float32)
    assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(rob, geometry.triangulate_robust(K, R, t, kpu, inlier_px=2.0)))
    assert bool(rob.ok.all())
    # zero coefficients: the call without dist, bit for bit
    zero = geometry.triangulate_triage(K, R, t, kp, dist=np.zeros(14))
    assert all(host(a).tobytes() == host(b).tobytes() for a, b in zip(zero, geometry.triangulate_triage(K, R, t, kp)))


def test_line_straightness_on_the_device():
    K, d, _ = lc.fixture_calibration()
    res = calibration.line_straightness(lc.checkerboards(K, d), (9, 6), K, d)
    assert res["straightness_rms_before_px"] > 0.5 and res["straightness_rms_after_px"] < 1e-8


# ---- the entry points on the tiny model, as tests/test_entry_points_gpu.py builds it -----------------------------------------
@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    return m


def _clip_pt(path, name, frames, kps, boxes):
    T, H, Wd = frames.shape[:3]
    torch.save({"video_name": name, "video_path": f"/videos/{name}.mp4", "frame_count": T, "img_shape": (H, Wd), "fps": 30,
                "detectron2": {"bbox": torch.from_numpy(boxes), "keypoints": torch.from_numpy(kps), "keypoints_score": torch.ones(T, 17)},
                "depth": torch.zeros(T, 1, 4, 4), "frames": frames}, path)


def _zero_calibration(path, golden_dir):
    with np.load(golden_dir / "calibration.npz") as z:
        np.savez(path, camera_matrix=z["camera_matrix"], dist_coeffs=np.zeros((1, 14)), image_size=z["image_size"])
    return path


def _same_npz(a, b):
    za, zb = np.load(a), np.load(b)
    return sorted(za.files) == sorted(zb.files) and all(za[k].tobytes() == zb[k].tobytes() and za[k].dtype == zb[k].dtype for k in za.files)


def test_multi_view_entry_point_with_the_lens_stage(tiny, tmp_path, golden_dir, caplog):
    rng = np.random.default_rng(1)
    T, H, Wd = 3, 135, 240
    lf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    rf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    lk = (rng.random((T, 17, 2)) * [Wd - 10, H - 10] + 5).astype(np.float32)
    rk = (rng.random((T, 17, 2)) * [Wd - 10, H - 10] + 5).astype(np.float32)
    lb = np.tile(np.array([[20, 10, 220, 125]], np.float32), (T, 1))
    rb = np.tile(np.array([[50, 20, 170, 120]], np.float32), (T, 1))
    (tmp_path / "subj").mkdir()
    _clip_pt(tmp_path / "subj" / "left.pt", "left", lf, lk, lb)
    _clip_pt(tmp_path / "subj" / "right.pt", "right", rf, rk, rb)
    head = infer.CameraHead({"infer": {"gpu": 0}}, None, model=tiny)
    zero = str(_zero_calibration(tmp_path / "zero.npz", golden_dir))
    real = str(golden_dir / "calibration_parameters.yml")
    runs = {"absent": {"hflip": True}, "off": {"hflip": True, "undistort": False, "calibration": real},
            "zero": {"hflip": True, "undistort": True, "calibration": zero},
            "real": {"hflip": True, "undistort": True, "calibration": [real, str(golden_dir / "calibration.npz")]}}
    out = {}
    for name, icfg in runs.items():
        head.outdir = None
        with caplog.at_level(logging.INFO, logger=mv.logger.name):
            mv.process_multi_view_video(tmp_path / "subj" / "left.mp4", tmp_path / "subj" / "left.pt", tmp_path / "subj" / "right.mp4",
                                        tmp_path / "subj" / "right.pt", tmp_path / name, tmp_path / name / "inf",
                                        {"infer": dict(icfg, gpu=0, triage=True)}, camera_head=head, steps_per_call=2)
        out[name] = tmp_path / name / "inf" / "subj_multi_view_3d_info.npz"
    assert _same_npz(out["absent"], out["off"]) and _same_npz(out["absent"], out["zero"])
    za, zr = np.load(out["absent"]), np.load(out["real"])
    assert sorted(za.files) == sorted(zr.files)
    assert zr["x3d"].shape == (T, 17, 3) and np.isfinite(zr["x3d"]).all() and not np.array_equal(zr["x3d"], za["x3d"])
    assert not np.array_equal(zr["R"], za["R"])                  # the frames the model saw changed too
    assert "largest resid_px" in caplog.text
    with pytest.raises(ValueError, match="calibration"):
        mv.process_multi_view_video(tmp_path / "subj" / "left.mp4", tmp_path / "subj" / "left.pt", tmp_path / "subj" / "right.mp4",
                                    tmp_path / "subj" / "right.pt", tmp_path / "x", tmp_path / "x" / "inf",
                                    {"infer": {"undistort": True}}, camera_head=head)
    # the detections the stage hands on: keypoints as the restatement moves them, boxes around their undistorted corners
    cal = lc.fixture_calibration()
    K = cal[0].copy()
    K[0] *= Wd / cal[2][0]
    K[1] *= H / cal[2][1]
    k2, b2, worst, lost = infer.undistort_detections(lk, lb, K, cal[1], head.device)
    want = lr.undistort_points(lk.astype(np.float64), K, cal[1])[0]
    assert k2.dtype == np.float32 and np.abs(k2 - want).max() < 1e-4 and worst < 1e-6 and lost == 0
    corners = lr.undistort_points(np.array([[20, 10], [220, 10], [20, 125], [220, 125.0]]), K, cal[1])[0]
    assert b2.shape == lb.shape and np.abs(b2[0] - np.r_[corners.min(0), corners.max(0)]).max() < 1e-4
    assert abs(b2[0, 0] - 20) > 1 and abs(b2[0, 2] - 220) > 1   # the box really moved


def test_single_view_entry_point_with_the_lens_stage(tiny, tmp_path, golden_dir):
    rng = np.random.default_rng(4)
    T, H, Wd = 35, 135, 240                         # frames 0, 30 -> S = 2
    fr = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    k = (rng.random((T, 17, 2)) * [Wd, H]).astype(np.float32)
    (tmp_path / "skier").mkdir()
    _clip_pt(tmp_path / "skier" / "cam.pt", "cam", fr, k, np.tile(np.array([[0, 0, 10, 10]], np.float32), (T, 1)))
    head = infer.CameraHead(None, None, model=tiny)
    zero = str(_zero_calibration(tmp_path / "zero.npz", golden_dir))
    runs = {"absent": {}, "off": {"undistort": False}, "zero": {"undistort": True, "calibration": zero},
            "real": {"undistort": True, "calibration": str(golden_dir / "calibration.npz")}}
    out = {}
    for name, icfg in runs.items():
        head.outdir = None
        sv.process_single_view_video(tmp_path / "skier" / "cam.mp4", tmp_path / "skier" / "cam.pt", tmp_path / name, tmp_path / name / "inf",
                                     {"infer": dict(icfg, gpu=0)}, camera_head=head)
        out[name] = tmp_path / name / "inf" / "skier_multi_view_3d_info.npz"
    assert _same_npz(out["absent"], out["off"]) and _same_npz(out["absent"], out["zero"])
    za, zr = np.load(out["absent"]), np.load(out["real"])
    assert sorted(za.files) == sorted(zr.files) and np.isfinite(zr["R"]).all() and not np.array_equal(zr["R"], za["R"])
