"""GPU: the bundle-adjustment kernel (csrc/ba.hip; geometry.bundle_adjust) against the float64 autograd restatement of
tests/ba_restated.py, and the opt-in stage of process_multi_view_video (cfg.infer.ba; the commented-out bundle
adjustment of vggt/multi_view_process.py:321-353).

Measured worst cases on an MI355X (T = 16, C = 2, J = 17, 200 iterations, all three modes): |d| / (1 + |x|) on R, t
and X = 5.5e-16 at lr 1e-3 and 7.9e-13 at lr 1e-2; relative on the history 2.3e-14 at lr 1e-3 and 1.2e-11 at lr 1e-2
(bounds: 1e-9 and 1e-10)."""
import json

import numpy as np
import pytest
import torch

import ba_restated as ref
from skiing_analysis_pytorch_amd import geometry, infer, vggt, weights as W
from skiing_analysis_pytorch_amd import multi_view_process as mv
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu

MODES = ("pose_only", "pose_cam_t", "full")


def _clip(T, C, J, seed=0, cam_noise=0.02, joint_noise=0.02, px_noise=2.0):
    """C cameras on a ring (radius 4) looking at a person near the origin; keypoints = projections of the true joints +
    pixel noise; the returned cameras and joints are perturbed."""
    rng = np.random.default_rng(seed)
    K = np.zeros((C, 3, 3))
    K[:, 0, 0], K[:, 1, 1] = rng.uniform(900, 1100, C), rng.uniform(900, 1100, C)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 960 + rng.normal(0, 5, C), 540 + rng.normal(0, 5, C), 1.0
    R, t, R_true, t_true = (np.zeros((T, C, 3, 3)), np.zeros((T, C, 3)), np.zeros((T, C, 3, 3)), np.zeros((T, C, 3)))
    for c in range(C):
        a = 2 * np.pi * c / max(C, 1) + 0.3
        ctr = np.array([4 * np.sin(a), -0.3, -4 * np.cos(a)])
        z = -ctr / np.linalg.norm(ctr)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        Rc = np.stack([x, np.cross(z, x), z])
        R_true[:, c], t_true[:, c] = Rc, -Rc @ ctr
        for s in range(T):
            ang = rng.normal(0, cam_noise, 3)
            R[s, c] = _exp(ang) @ Rc
            t[s, c] = -R[s, c] @ (ctr + rng.normal(0, cam_noise, 3))
    X_true = rng.normal(0, 0.4, (J, 3)) + np.cumsum(rng.normal(0, 0.01, (T, J, 3)), 0)
    Xc = np.einsum("tcij,tkj->tcki", R_true, X_true) + t_true[:, :, None]
    x2d = np.einsum("cij,tckj->tcki", K, Xc / Xc[..., 2:3])[..., :2] + rng.normal(0, px_noise, (T, C, J, 2))
    conf = rng.uniform(0.3, 1.0, (T, C, J))
    X = X_true + rng.normal(0, joint_noise, X_true.shape)
    return K, R, t, X, x2d, conf


def _exp(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th**2 * Kx @ Kx


def _errs(res, want):
    R, t, X, h = want
    e = max(float((np.abs(g.cpu().numpy() - w.numpy()) / (1 + np.abs(w.numpy()))).max())
            for g, w in ((res.R, R), (res.t, t), (res.X, X)))
    hw = h.numpy()
    eh = float((np.abs(res.history.cpu().numpy() - hw) / np.maximum(np.abs(hw), 1e-300)).max()) if hw.size else 0.0
    return e, eh


def _check(clip, modes=MODES, num_iters=200, lr=1e-3, weights=None, tol=1e-9, htol=1e-10, **kw):
    res = geometry.bundle_adjust(*clip, modes=modes, num_iters=num_iters, lr=lr, weights=weights, **kw)
    worst = (0.0, 0.0)
    for r in res:
        want = ref.run(*clip, mode=r.mode, num_iters=num_iters, lr=lr, weights=weights)
        e, eh = _errs(r, want)
        assert e <= tol, (r.mode, e)
        assert eh <= htol, (r.mode, eh)
        worst = (max(worst[0], e), max(worst[1], eh))
    return res, worst


@pytest.mark.parametrize("lr", [1e-3, 1e-2])
def test_modes_match_restatement(lr):
    clip = _clip(16, 2, 17, seed=1)
    res, worst = _check(clip, lr=lr)
    print(f"lr {lr}: worst |d|/(1+|x|) {worst[0]:.2e}, history {worst[1]:.2e}")
    assert [r.mode for r in res] == list(MODES)
    # the optimisation moved what each mode optimises
    X0 = clip[3]
    for r in res:
        assert not np.array_equal(r.X.cpu().numpy(), X0)
    assert not np.array_equal(res[1].t.cpu().numpy(), clip[2]) and not np.array_equal(res[2].R.cpu().numpy(), clip[1])


@pytest.mark.parametrize("T,C,J", [(1, 2, 17), (2, 2, 17), (16, 1, 17), (16, 3, 17), (16, 2, 12), (8, 3, 12)])
def test_edge_shapes_match_restatement(T, C, J):
    clip = _clip(T, C, J, seed=T * 100 + C * 10 + J)
    res, _ = _check(clip, lr=1e-2, weights={"ba_weight_smooth": 0.1, "ba_weight_bone_length": 0.1,
                                            "ba_weight_pose_temporal": 0.1})
    h = res[0].history.cpu().numpy()
    if T == 1:
        assert (h[:, 2] == 0).all() and (h[:, 5] == 0).all()
    if C == 1:
        assert (h[:, 3] == 0).all()
    assert np.isfinite(h).all()


def test_zero_conf_joint_and_joint_behind_a_camera():
    K, R, t, X, x2d, conf = _clip(6, 3, 17, seed=7)
    conf[:, :, 4] = 0.0                                            # joint 4: conf 0 in every view
    X[2, 3] = -(R[2, 2].T @ t[2, 2]) - 0.1 * R[2, 2][2]           # joint 3 of step 2 behind camera 2: Z clamped
    Zc = (R[2, 2] @ X[2, 3] + t[2, 2])[2]
    assert Zc < 0
    _check((K, R, t, X, x2d, conf), lr=1e-2)


def test_state_outside_lds_matches_restatement():
    """T = 4096: the state does not fit in LDS and lives in the workspace."""
    clip = _clip(4096, 2, 17, seed=11)
    assert int(geometry.lib().skimi_ba_workspace_bytes(4096, 2, 17, 1)) > 160 * 1024
    _check(clip, num_iters=20, lr=1e-2)
    with pytest.raises(geometry._lib.SkimiError, match="does not fit in LDS"):
        geometry.bundle_adjust(*clip, modes="pose_only", num_iters=1, placement="lds")


def _bits(res):
    return [(r.R.cpu().numpy().tobytes(), r.t.cpu().numpy().tobytes(), r.X.cpu().numpy().tobytes(),
             r.history.cpu().numpy().tobytes()) for r in res]


def test_one_launch_equals_single_launches_and_reruns():
    clip = _clip(16, 2, 17, seed=3)
    kw = dict(num_iters=200, lr=1e-2)
    together = _bits(geometry.bundle_adjust(*clip, modes=MODES, **kw))
    alone = [_bits(geometry.bundle_adjust(*clip, modes=m, **kw))[0] for m in MODES]
    assert together == alone
    assert _bits(geometry.bundle_adjust(*clip, modes=MODES, **kw)) == together
    # the placement of the state does not change the results
    assert _bits(geometry.bundle_adjust(*clip, modes=MODES, placement="workspace", **kw)) == together
    assert _bits(geometry.bundle_adjust(*clip, modes=MODES, placement="lds", **kw)) == together


def test_blocks_a_mode_does_not_optimise_are_the_inputs():
    K, R, t, X, x2d, conf = _clip(16, 2, 17, seed=4)
    po, pt, full = geometry.bundle_adjust(K, R, t, X, x2d, conf, modes=MODES, num_iters=50, lr=1e-2)
    assert po.R.cpu().numpy().tobytes() == R.tobytes() and po.t.cpu().numpy().tobytes() == t.tobytes()
    assert pt.R.cpu().numpy().tobytes() == R.tobytes()
    # zero iterations: every block is its input
    for r in geometry.bundle_adjust(K, R, t, X, x2d, conf, modes=MODES, num_iters=0):
        assert r.history.shape == (0, 6)
        assert (r.R.cpu().numpy().tobytes(), r.t.cpu().numpy().tobytes(), r.X.cpu().numpy().tobytes()) == \
            (R.tobytes(), t.tobytes(), X.tobytes())


def test_ring_rig_reprojection_decreases():
    clip = _clip(32, 4, 17, seed=5, cam_noise=0.03, joint_noise=0.05)
    w = {"ba_weight_reproj": 1.0, "ba_weight_smooth": 0.1, "ba_weight_baseline": 0.01, "ba_weight_bone_length": 0.1,
         "ba_weight_pose_temporal": 0.1}     # configs/vggt.yaml:43-51
    for r in geometry.bundle_adjust(*clip, modes=MODES, num_iters=2000, lr=1e-2, weights=w):
        h = r.history.cpu().numpy()
        assert np.isfinite(h).all()
        assert h[-1, 1] < 0.5 * h[0, 1], (r.mode, h[0, 1], h[-1, 1])
        assert h[-1, 0] < h[0, 0]


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    return m


def _clip_pt(path, name, frames, kps, scores, boxes):
    T, H, Wd = frames.shape[:3]
    torch.save({"video_name": name, "video_path": f"/videos/{name}.mp4", "frame_count": T, "img_shape": (H, Wd), "fps": 30,
                "detectron2": {"bbox": torch.from_numpy(boxes), "keypoints": torch.from_numpy(kps),
                               "keypoints_score": torch.from_numpy(scores)},
                "depth": torch.zeros(T, 1, 4, 4), "frames": frames}, path)


def test_process_multi_view_video_with_ba(tiny, tmp_path):
    rng = np.random.default_rng(2)
    T, H, Wd = 3, 135, 240
    lf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    rf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    lk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    rk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    ls = rng.uniform(0.2, 1.0, (T, 17)).astype(np.float32)
    rs = rng.uniform(0.2, 1.0, (T, 17)).astype(np.float32)
    lb = np.tile(np.array([[60, 30, 180, 110]], np.float32), (T, 1))
    rb = np.tile(np.array([[50, 20, 170, 120]], np.float32), (T, 1))
    (tmp_path / "subj").mkdir()
    _clip_pt(tmp_path / "subj" / "left.pt", "left", lf, lk, ls, lb)
    _clip_pt(tmp_path / "subj" / "right.pt", "right", rf, rk, rs, rb)
    head = infer.CameraHead({"infer": {"gpu": 0}}, None, model=tiny)
    z = {}
    for ba in (False, True):
        out = tmp_path / f"ba{int(ba)}"
        cfg = {"infer": {"gpu": 0, "ba": ba}, "bundle_adjustment": {"num_iters": 50, "lr": 1e-2, "ba_weight_smooth": 0.1}}
        mv.process_multi_view_video(tmp_path / "subj" / "left.mp4", tmp_path / "subj" / "left.pt", tmp_path / "subj" / "right.mp4",
                                    tmp_path / "subj" / "right.pt", out, out / "inf", cfg, camera_head=head, steps_per_call=2)
        z[ba] = dict(np.load(out / "inf" / "subj_multi_view_3d_info.npz"))
    off, on = z[False], z[True]
    ba_keys = sorted(k for k in on if k.startswith("ba_"))
    assert ba_keys == sorted(f"ba_{m}_{f}" for m in MODES for f in ("x3d", "R", "t", "history"))
    assert sorted(k for k in on if not k.startswith("ba_")) == sorted(off)
    for k in off:
        assert on[k].dtype == off[k].dtype and on[k].tobytes() == off[k].tobytes(), k
    # the ba_* keys are geometry.bundle_adjust of the NPZ's own arrays
    x2d = np.stack([np.stack([lk[i], rk[i]]) for i in range(T)]).astype(np.float64)
    conf = np.stack([np.stack([ls[i], rs[i]]) for i in range(T)]).astype(np.float64)
    res = geometry.bundle_adjust(on["camera_intrinsics"].astype(np.float64).mean(0), on["R"], on["t"], on["x3d"], x2d, conf,
                                 modes=MODES, num_iters=50, lr=1e-2, weights={"ba_weight_smooth": 0.1})
    for r in res:
        for f, v in (("x3d", r.X), ("R", r.R), ("t", r.t), ("history", r.history)):
            assert on[f"ba_{r.mode}_{f}"].tobytes() == v.cpu().numpy().tobytes(), (r.mode, f)
    # run_local_ba: the reference caller's keywords (:553-564) and tuple
    R_opt, t_opt, X_opt, history = mv.run_local_ba(
        K_torch=torch.from_numpy(on["camera_intrinsics"].astype(np.float64).mean(0)), R_init_torch=torch.from_numpy(on["R"]),
        t_init_torch=torch.from_numpy(on["t"]), X3d_init_torch=torch.from_numpy(on["x3d"]),
        x2d_torch=torch.from_numpy(x2d).float(), conf2d_torch=torch.from_numpy(conf).float(), num_iters=50, lr=1e-2,
        device="cuda", mode="pose_cam_t")
    assert X_opt.shape == (T, 17, 3) and R_opt.shape == (T, 2, 3, 3) and t_opt.shape == (T, 2, 3)
    assert history.shape == (50, 6) and X_opt.dtype == torch.float64 and X_opt.is_cuda
    want = geometry.bundle_adjust(on["camera_intrinsics"].astype(np.float64).mean(0), on["R"], on["t"], on["x3d"],
                                  torch.from_numpy(x2d).float(), torch.from_numpy(conf).float(), modes="pose_cam_t",
                                  num_iters=50, lr=1e-2)[0]
    assert X_opt.cpu().numpy().tobytes() == want.X.cpu().numpy().tobytes()
    assert t_opt.cpu().numpy().tobytes() == want.t.cpu().numpy().tobytes()
