"""CPU: the float64 restatement of the lens model (tests/lens_restated.py), which the GPU tests hold csrc/lens.hip against,
is itself held against the reference's cv2-free distortion.py (tests/golden/lens.npz, tools/make_goldens.py gen_lens) and
against the properties the model must have on the rig's own calibration (tests/golden/calibration.npz): it round-trips over
the whole 1920 x 1080 frame, five iterations already agree with twenty, and the displacement is the 25.5 px that makes the
feature necessary.  Then the image restatement's identities, the calibration loader and the host checks of calibration.py."""
import numpy as np
import pytest

import lens_cases as lc
import lens_restated as lr
from skiing_analysis_pytorch_amd import calibration, formats, geometry

GOLD = np.load(lc.GOLDEN / "lens.npz")


def per_row(fn, params, *cols):
    return np.stack([np.stack(fn(*[c[b] for c in cols], params[b]), -1) for b in range(len(params))])


@pytest.mark.parametrize("name,pad", [("p1", lambda p: np.c_[p, np.zeros((len(p), 3))]), ("p2", lambda p: np.c_[p, np.zeros((len(p), 2))]),
                                      ("p4", lambda p: p)])
def test_forward_model_matches_reference(name, pad):
    """apply_distortion's 1- and 2-parameter models are (k1, 0, 0, 0) and (k1, k2, 0, 0) of its OpenCV model.  Bound 1e-12
    (measured 2e-16): both sides are a dozen float64 operations on values below 1."""
    params = pad(GOLD[f"fwd_{name}_params"])
    got = per_row(lr.distort_normalized, params, GOLD["fwd_u"], GOLD["fwd_v"])
    err = np.abs(got - GOLD[f"fwd_{name}"]).max()
    print(f"forward {name}: max abs difference {err:.3g}")
    assert err <= 1e-12


def test_inverse_matches_reference_inside_invertible_range():
    """iterative_undistortion stops at a step of 1e-5 and carries an error of that size, which the generator measured against
    the truth and stored; the fixed-point inverse is exact to rounding, so the two differ by the reference's error: the
    bound is 1.5 x the stored value."""
    truth = GOLD["inv_truth"]
    assert ((truth ** 2).sum(-1) <= lc.REF_INVERTIBLE_R2).all()
    x, y = lr.undistort_normalized(GOLD["inv_distorted"][0, :, 0], GOLD["inv_distorted"][0, :, 1], GOLD["inv_params"][0], iters=200)
    ours = np.abs(np.stack([x, y], -1) - truth[0]).max()
    diff = np.abs(np.stack([x, y], -1) - GOLD["inv_undistorted"][0]).max()
    ref_err = float(GOLD["inv_ref_err"])
    print(f"inverse: ours vs truth {ours:.3g}, ours vs reference {diff:.3g}, reference vs truth (stored) {ref_err:.3g}")
    assert 0 < ref_err < 5e-5
    assert ours <= 1e-12
    assert diff <= 1.5 * ref_err


def test_round_trip_over_the_whole_frame_with_the_rig_calibration():
    K, d, (w, h) = lc.fixture_calibration()
    assert (w, h) == (1920, 1080) and d.size == 14 and abs(d[0] + 1.194) < 1e-3 and abs(d[4] - 98.84) < 1e-2
    px = lc.full_frame_grid(w, h)
    u20, r20 = lr.undistort_points(px, K, d, iters=20)
    u5, _ = lr.undistort_points(px, K, d, iters=5)
    back = lr.distort_points(u20, K, d)
    rt = np.linalg.norm(back - px, axis=-1).max()
    d5 = np.linalg.norm(u5 - u20, axis=-1).max()
    disp = np.linalg.norm(u20 - px, axis=-1).max()
    print(f"round trip {rt:.3g} px, resid_px max {r20.max():.3g}, iters 5 vs 20 {d5:.3g} px, largest displacement {disp:.4f} px")
    assert rt <= 1e-9 and r20.max() <= 1e-9
    assert d5 <= 1e-6
    assert 25.0 < disp < 26.0
    # normalised output and P: the same point in other units
    un, _ = lr.undistort_points(px, K, d, normalized=True)
    P = lc.small_K(w, h)
    up, _ = lr.undistort_points(px, K, d, P=P)
    assert np.abs(up - (un * [P[0, 0], P[1, 1]] + [P[0, 2], P[1, 2]])).max() <= 1e-9
    assert np.abs(lr.distort_points(un, K, d, normalized=True) - px).max() <= 1e-9
    assert np.abs(lr.distort_points(up, K, d, P=P) - px).max() <= 1e-9


def test_point_beyond_the_fold_over_is_exposed_by_resid_px():
    K = lc.small_K(1920, 1080, 0.58)
    x = np.array([lc.FOLD_POINT_NORMALIZED]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    inside = np.array([[0.3, 0.2]]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    _, resid = lr.undistort_points(np.r_[x, inside], K, lc.REF_P4[0])
    print("resid_px beyond the fold-over and inside:", resid)
    assert np.isnan(resid[0]) or resid[0] > 1.0
    assert resid[1] < 1e-9


def test_nan_keypoint_and_projection():
    K, d, _ = lc.fixture_calibration()
    px = lc.full_frame_grid()[:5].copy()
    px[2, 1] = np.nan
    u, r = lr.undistort_points(px, K, d)
    assert np.isnan(u[2]).all() and np.isnan(r[2]) and np.isfinite(np.delete(u, 2, 0)).all() and np.isfinite(np.delete(r, 2)).all()
    # projection without coefficients is the pinhole, with them it is distort_points of the pinhole pixel
    rig = lc.rig_case()
    X, R, t, K0 = rig["X"][0], rig["R"][0, 1], rig["t"][0, 1], rig["K"][0, 1]
    pin, depth = lr.project_points(X, R, t, K0)
    cam = X @ R.T + t
    assert np.abs(pin - (cam @ K0.T)[:, :2] / cam[:, 2:]).max() < 1e-9 and np.abs(depth - cam[:, 2]).max() < 1e-12
    assert np.abs(lr.project_points(X, R, t, K0, d)[0] - lr.distort_points(pin, K0, d)).max() < 1e-9


@pytest.fixture(scope="module")
def frames():
    out = {}
    for name, case in lc.image_cases().items():
        imgs = lc.images_of(case)
        out[name] = (case, imgs) + lc.restated_frames(case, imgs)
    return out


def test_image_restatement_identity_shift_and_near_ties(frames):
    case = lc.image_cases()["37x53"]
    img = lc.images_of(case)[0, 0]
    K = case["K"][0]
    assert np.array_equal(lr.undistort_image(img, K, np.zeros(4)), img)
    newK = K.copy()
    newK[0, 2] += 5          # the output's principal point 5 px right and 3 px up: the picture moves with it
    newK[1, 2] -= 3
    want = np.zeros_like(img)
    want[:-3, 5:] = img[3:, :-5]
    assert np.array_equal(lr.undistort_image(img, K, np.zeros(5), newK), want)
    for name, (case, imgs, out, tie) in frames.items():
        share = tie.mean()
        print(f"{name}: near-tie share {share:.3g} of {tie.size} values, output mean {out.mean():.1f}")
        assert share <= 1e-5
        assert out.shape == imgs.shape[:2] + ((case["out_size"] or (case["W"], case["H"]))[::-1]) + (case["ch"],)
    assert frames["270x480_fixture"][2].std() > 20      # a picture, not a border


def test_load_calibration_reads_both_formats():
    a = formats.load_calibration(lc.GOLDEN / "calibration.npz")
    b = formats.load_calibration(lc.GOLDEN / "calibration_parameters.yml")
    K, d, size = lc.fixture_calibration()
    for c in (a, b):
        assert c.image_size == (1920, 1080) == size and c.K.dtype == np.float64 and c.K.shape == (3, 3) and c.dist.shape == (14,)
        assert np.array_equal(c.K, K) and np.array_equal(c.dist, d)
    s = a.scaled_to(480, 270)
    assert s.image_size == (480, 270) and np.array_equal(s.dist, a.dist)
    assert np.allclose(s.K, [[K[0, 0] / 4, 0, K[0, 2] / 4], [0, K[1, 1] / 4, K[1, 2] / 4], [0, 0, 1]], rtol=1e-15, atol=0)
    assert np.array_equal(a.scaled_to(1920, 1080).K, K)
    with pytest.raises(ValueError, match="aspect"):
        a.scaled_to(480, 360)
    with pytest.raises(ValueError):
        formats.load_calibration(lc.GOLDEN / "lens.npz")          # no camera_matrix: refused, and never unpickled


def test_load_calibration_yaml_short_vector(tmp_path):
    p = tmp_path / "c.yml"
    p.write_text("%YAML:1.0\n---\nimage_width: 640\nimage_height: 480\ncamera_matrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n"
                 "   data: [ 500., 0., 320., 0., 501., 240., 0., 0., 1. ]\ndistortion_coefficients: !!opencv-matrix\n   rows: 1\n"
                 "   cols: 5\n   dt: d\n   data: [ -1.5e-01, 2.0e-02, 0., 1.0e-03,\n       -3.0e-03 ]\n")
    c = formats.load_calibration(p)
    assert c.image_size == (640, 480) and c.K[1, 1] == 501.0
    assert np.array_equal(c.dist, [-0.15, 0.02, 0, 0.001, -0.003] + [0] * 9)


def test_lens_coeffs_padding_and_tilt():
    for k, v in lc.COEFFS.items():
        d = geometry.lens_coeffs(v)
        assert d.shape == (12,) and np.array_equal(d, lr.pad_dist(v)) and np.array_equal(d[:min(k, 12)], v[:12])
    assert np.array_equal(geometry.lens_coeffs(None), np.zeros(12))
    assert geometry.lens_coeffs(np.zeros((1, 14))).shape == (12,)           # cv2's [1, k] layout
    with pytest.raises(ValueError, match="tilt"):
        geometry.lens_coeffs([0.1] * 12 + [0.0, 0.01])
    with pytest.raises(ValueError):
        geometry.lens_coeffs([0.1] * 6)


def test_line_straightness_and_fov():
    K, d, size = lc.fixture_calibration()
    boards = lc.checkerboards(K, d)
    res = calibration.line_straightness(boards, (9, 6), K, d, undistort=lambda x, K_, d_: lr.undistort_points(x, K_, d_)[0])
    print(res)
    assert res["straightness_rms_before_px"] > 0.5
    assert res["straightness_rms_after_px"] < 1e-8
    f = calibration.fov_and_principal(K, size)
    assert abs(f["hfov_deg"] - 2 * np.degrees(np.arctan(960 / K[0, 0]))) < 1e-12 and 80 < f["hfov_deg"] < 83 and 50 < f["vfov_deg"] < 53
    assert f["principal_point_offset_px"] == (K[0, 2] - 960, K[1, 2] - 540) and abs(f["aspect_fx_fy"] - 1) < 1e-3


def test_rig_needs_the_lens_on_the_restatement():
    """the premise of the GPU rig test, on the restatement: raw keypoints lose joints at 2 px, undistorted ones lose none"""
    import person_restated as pr
    from oracle import vggt_oracle

    rig = lc.rig_case()
    T, V, J = rig["kp"].shape[:3]
    assert rig["kp"][:, 0].min() < 2 and rig["kp"][:, 0, :, 0].max() > 1916          # the corners of camera 0's frame
    und = np.stack([[lr.undistort_points(rig["kp"][i, v], rig["K"][i, v], rig["dist"])[0] for v in range(V)] for i in range(T)])
    assert np.abs(und - rig["kp_ideal"]).max() < 1e-8
    for kp, all_kept in ((rig["kp"], False), (und.astype(np.float32).astype(np.float64), True)):
        X = np.stack([vggt_oracle.triangulate_one_frame(rig["K"][i], rig["R"][i], rig["t"][i], kp[i]) for i in range(T)])
        keep = pr.triage(rig["K"], rig["R"], rig["t"], kp, X)["keep"]
        print("kept", keep.sum(), "of", keep.size, "| max |X - truth|", np.abs(X - rig["X"]).max())
        assert keep.all() == all_kept
        if all_kept:
            assert np.abs(X - rig["X"]).max() < 1e-6
        else:
            assert (~keep).sum() >= 1
