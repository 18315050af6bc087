"""GPU: the point-to-plane ICP kernels (csrc/icp.hip; geometry.estimate_normals / icp_correspondences /
icp_point_to_plane) against the float64 restatement of tests/icp_restated.py, and the opt-in refinement of
process_multi_view_video (cfg.infer.icp, vggt/multi_view_process.py:263-291)."""
import json

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import icp_restated as ref
from skiing_analysis_pytorch_amd import geometry, infer, vggt, weights as W
from skiing_analysis_pytorch_amd import multi_view_process as mv
from skiing_analysis_pytorch_amd._lib import PREC_BF16X3

pytestmark = pytest.mark.gpu


def _motion(deg, axis, trans):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.deg2rad(deg) * np.asarray(axis, float) / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = trans
    return T


def _surface(n=120, spacing=0.011, seed=0, extent_z=1.0):
    """jittered lattice on a smooth non-planar surface: ~60-80 neighbours per 0.05 ball"""
    rng = np.random.default_rng(seed)
    u = (np.arange(n) - n / 2) * spacing
    x, y = np.meshgrid(u, u, indexing="ij")
    x = x + rng.uniform(-0.3, 0.3, x.shape) * spacing
    y = y + rng.uniform(-0.3, 0.3, y.shape) * spacing
    z = 0.12 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y) + 0.08 * x * y + extent_z
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def _moved(P, M, noise=0.0, seed=1):
    Minv = np.linalg.inv(M)
    Q = P.astype(np.float64) @ Minv[:3, :3].T + Minv[:3, 3]
    if noise:
        Q = Q + np.random.default_rng(seed).normal(scale=noise, size=Q.shape)
    return Q.astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _check_normals(P, radius=0.05):
    n_gpu, c_gpu = geometry.estimate_normals(_dev(P), radius)
    n_gpu, c_gpu = n_gpu.cpu().numpy(), c_gpu.cpu().numpy()
    v = ref.valid_mask(P)
    n_ref, c_ref = ref.normals(P[v], radius)
    assert np.array_equal(c_gpu[v], c_ref)
    assert (c_gpu[~v] == 0).all() and (n_gpu[~v] == 0).all()
    many = c_ref >= 3
    assert np.abs(np.einsum("ij,ij->i", n_gpu[v][many], n_ref[many])).min() >= 1 - 1e-9
    assert np.array_equal(n_gpu[v][~many], n_ref[~many])     # (0, 0, 1)
    return c_ref


def _check_icp(src, tgt, **kw):
    got = geometry.icp_point_to_plane(_dev(src), _dev(tgt), **kw)
    T, fit, rmse, it = ref.icp_point_to_plane(src, tgt, **kw)
    assert got.iterations == it, (got.iterations, it)
    assert got.fitness == fit
    assert abs(got.inlier_rmse - rmse) <= 1e-9 * max(rmse, 1e-300)
    assert np.abs(got.transformation - T).max() <= 1e-9, np.abs(got.transformation - T).max()
    return got


def test_normals_match_restatement_with_invalid_and_isolated_points():
    P = _surface(100)
    rng = np.random.default_rng(7)
    bad = rng.choice(len(P), 300, replace=False)
    P[bad[:100]] = 0.0
    P[bad[100:200], rng.integers(0, 3, 100)] = np.nan
    P[bad[200:250], 0] = np.inf
    P[bad[250:], 2] = -np.inf
    iso = np.array([[5, 5, 5], [-5, 5, 5], [-5, 5, 5.02], [3, -3, 3], [3.01, -3, 3], [3, -2.99, 3], [1e9, -2e9, 3e9]], np.float32)
    P = np.concatenate([P, iso])
    c = _check_normals(P)
    assert c.max() >= 40 and (c == 1).sum() >= 2 and (c == 2).sum() >= 2 and (c == 3).sum() >= 3
    # a sphere cap and far-away isolated background points (coordinates beyond the grid's clamp)
    th = np.deg2rad(np.linspace(0.5, 15, 60))
    ph = np.linspace(0, 2 * np.pi, 500, endpoint=False)
    T_, P_ = np.meshgrid(th, ph, indexing="ij")
    S = (np.stack([np.sin(T_) * np.cos(P_), np.sin(T_) * np.sin(P_), np.cos(T_)], -1).reshape(-1, 3) * 1.5).astype(np.float32)
    far = (rng.uniform(-1, 1, size=(200, 3)) * 1e5 + [2e5, -1e6, 7e4]).astype(np.float32)
    _check_normals(np.concatenate([S, far]))


def test_correspondences_match_restatement():
    tgt = _surface(110)
    src = _moved(_surface(110, seed=3), _motion(1.5, (0.2, 1, 0.1), (0.01, 0.0, -0.006)))
    src[::97] = np.nan
    tgt[::89] = 0.0
    for T in (np.eye(4), _motion(1.0, (1, 0, 0.3), (0.004, 0.002, -0.003)), _motion(0.0, (1, 0, 0), (0.2, 0, 0))):
        got = geometry.icp_correspondences(_dev(src), _dev(tgt), T, 0.05).cpu().numpy()
        want = ref.correspondences(src, tgt, T, 0.05)
        assert np.array_equal(got, want)
        assert (want >= 0).sum() > 100


def test_correspondence_ties_and_boundary():
    h = 2.0 ** -6    # exact in float32: equidistant targets in different grid cells
    s = np.array([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [0.25, 0.25, 0.25], [0.75, 0.75, 0.75]], np.float32)
    tgt = np.array([
        [0.5 + h, 0.5, 0.5], [0.5, 0.5 - h, 0.5], [0.5 - h, 0.5, 0.5], [0.5, 0.5, 0.5 + h],   # 4 ties for s0 -> 0
        [1.0, 1.0, 1.0 + h], [1.0, 1.0 - h, 1.0], [9, 9, 9], [1.0 - h, 1.0, 1.0],            # 3 ties for s1 -> 4
        [0.25 + 0.05 - 2e-6, 0.25, 0.25],                                                     # just inside for s2
        [0.75 + 0.05 + 2e-6, 0.75, 0.75], [0.75, 0.75 - 0.05 - 2e-6, 0.75],                   # just outside for s3
    ], np.float32)
    # the same clouds with the tied targets in the reverse index order: the smaller index still wins
    order = np.array([3, 2, 1, 0, 7, 5, 6, 4, 8, 9, 10])
    for tg in (tgt, tgt[order]):
        got = geometry.icp_correspondences(_dev(s), _dev(tg), np.eye(4), 0.05).cpu().numpy()
        want = ref.correspondences(s, tg, np.eye(4), 0.05)
        assert np.array_equal(got, want)
    assert got.tolist() == [0, 4, 8, -1]
    d = tgt[8].astype(np.float64) - s[2]
    assert 0.05 - 3e-6 < np.sqrt(d @ d) < 0.05
    # under a translation that puts s2's neighbour just outside
    T = np.eye(4)
    T[0, 3] = -4e-6
    assert geometry.icp_correspondences(_dev(s), _dev(tgt), T, 0.05).cpu().numpy()[2] == -1
    assert ref.correspondences(s, tgt, T, 0.05)[2] == -1


@pytest.mark.parametrize("deg,axis,trans", [(2.0, (0.3, 1, 0.2), (0.01, -0.005, 0.004)), (1.2, (1, -0.4, 0.7), (-0.006, 0.008, 0.0))])
def test_icp_matches_restatement_on_smooth_surfaces(deg, axis, trans):
    tgt = _surface(110)
    M = _motion(deg, axis, trans)
    src = _moved(_surface(110, seed=11), M)             # another sampling of the same surface
    got = _check_icp(src, tgt)
    assert got.fitness > 0.9 and got.iterations > 2
    assert np.abs(got.transformation[:3, :3] - M[:3, :3]).max() < 2e-3   # a different sampling: close, not exact
    # the same sampling: the motion itself
    exact = _check_icp(_moved(tgt, M), tgt)
    assert np.abs(exact.transformation - M).max() < 1e-6


def test_icp_iteration_cap_no_correspondences_few_points_and_init():
    tgt = _surface(90)
    M = _motion(2.0, (0.5, 1, -0.3), (0.01, 0.004, -0.008))
    src = _moved(_surface(90, seed=5), M, noise=1e-3)
    got = _check_icp(src, tgt, max_iteration=3)
    assert got.iterations == 3
    # init != I
    init = _motion(1.0, (0.5, 1, -0.3), (0.005, 0.002, -0.004))
    _check_icp(src, tgt, init=init, max_iteration=50)
    # no correspondences: identity after one update of the identity, fitness 0
    far = tgt + np.float32(10.0)
    got = _check_icp(src, far)
    assert np.array_equal(got.transformation, np.eye(4)) and got.fitness == 0 and got.inlier_rmse == 0
    # fewer than 50 valid points: identity, 0 iterations
    few = np.concatenate([tgt[:49], np.full((30, 3), np.nan, np.float32), np.zeros((30, 3), np.float32)])
    for a, b in ((few, tgt), (src, few)):
        got = _check_icp(a, b)
        assert np.array_equal(got.transformation, np.eye(4)) and got.iterations == 0 and got.fitness == 0


@pytest.fixture(scope="module")
def tiny(golden_dir):
    g = np.load(golden_dir / "vggt_tiny_conv.npz")
    cfg = W.VGGTConfig(**json.loads(str(g["cfg_json"])))
    m = vggt.VGGT(config=cfg, prec=PREC_BF16X3, head_prec=PREC_BF16X3)
    m.load_state_dict(W.make_vggt_state_dict(cfg, seed=0))
    return m


def test_icp_on_tiny_vggt_world_points(tiny):
    images = W.make_images(2, 140, 140, seed=21).cuda()[None]
    with torch.no_grad():
        out = tiny(images, want={"camera", "depth"})
    E, K = geometry.pose_encoding_to_extri_intri(out["pose_enc"], (140, 140))
    wp = geometry.unproject_depth_map_to_point_map(out["depth"][0], E[0], K[0]).cpu().numpy()
    _check_icp(wp[0].reshape(-1, 3), wp[1].reshape(-1, 3))


def _full_size_pair():
    """two 518 x 518 maps (268 324 points each) of a synthetic scene: a wavy ground, a few invalid pixels and far
    background points; the source is another sampling moved by a small motion"""
    n = 518
    tgt = _surface(n, spacing=0.0155, seed=31)
    M = _motion(1.5, (0.2, 1, 0.4), (0.008, -0.004, 0.006))
    src = _moved(_surface(n, spacing=0.0155, seed=32), M, noise=5e-4)
    rng = np.random.default_rng(33)
    for P in (src, tgt):
        P[rng.choice(len(P), 2000, replace=False)] = 0.0
        bg = rng.choice(len(P), 3000, replace=False)
        P[bg] = (rng.normal(size=(3000, 3)) * 40 + [0, 0, 300]).astype(np.float32)
    return src, tgt


def test_full_size_pair_and_determinism():
    src, tgt = _full_size_pair()
    assert len(src) == len(tgt) == 268324
    rng = np.random.default_rng(34)
    sample = rng.choice(len(tgt), 2000, replace=False)
    n_gpu, c_gpu = geometry.estimate_normals(_dev(tgt), 0.05)
    n_gpu, c_gpu = n_gpu.cpu().numpy(), c_gpu.cpu().numpy()
    v = ref.valid_mask(tgt)
    n_ref = np.zeros((len(tgt), 3))
    c_ref = np.zeros(len(tgt), np.int64)
    n_ref[v], c_ref[v] = ref.normals(tgt[v], 0.05)
    assert np.array_equal(c_gpu[sample], c_ref[sample])
    ok = sample[c_ref[sample] >= 3]
    assert len(ok) > 1500 and np.median(c_ref[ok]) >= 20
    assert np.abs(np.einsum("ij,ij->i", n_gpu[ok], n_ref[ok])).min() >= 1 - 1e-9
    T = _motion(0.5, (0, 1, 0), (0.003, 0, 0))
    got = geometry.icp_correspondences(_dev(src), _dev(tgt), T, 0.05).cpu().numpy()
    want = ref.correspondences(src, tgt, T, 0.05)
    assert np.array_equal(got[sample], want[sample])
    a = _check_icp(src, tgt, max_iteration=5)
    assert 1 < a.iterations <= 5 and a.fitness > 0.95
    assert _check_icp(src, tgt, max_iteration=2).iterations == 2
    b = geometry.icp_point_to_plane(_dev(src), _dev(tgt), max_iteration=5)
    assert np.array_equal(a.transformation, b.transformation)
    assert a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse


def _clip_pt(path, name, frames, kps, boxes):
    T, H, Wd = frames.shape[:3]
    torch.save({"video_name": name, "video_path": f"/videos/{name}.mp4", "frame_count": T, "img_shape": (H, Wd), "fps": 30,
                "detectron2": {"bbox": torch.from_numpy(boxes), "keypoints": torch.from_numpy(kps),
                               "keypoints_score": torch.ones(T, 17)},
                "depth": torch.zeros(T, 1, 4, 4), "frames": frames}, path)


def test_process_multi_view_video_with_icp(tiny, tmp_path):
    rng = np.random.default_rng(1)
    T, H, Wd = 2, 135, 240
    lf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    rf = torch.from_numpy(rng.integers(0, 256, (T, H, Wd, 3), dtype=np.uint8))
    lk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    rk = (rng.random((T, 17, 2)) * [Wd - 40, H - 40] + 20).astype(np.float32)
    lb = np.tile(np.array([[60, 30, 180, 110]], np.float32), (T, 1))
    rb = np.tile(np.array([[50, 20, 170, 120]], np.float32), (T, 1))
    (tmp_path / "subj").mkdir()
    _clip_pt(tmp_path / "subj" / "left.pt", "left", lf, lk, lb)
    _clip_pt(tmp_path / "subj" / "right.pt", "right", rf, rk, rb)
    head = infer.CameraHead({"infer": {"gpu": 0}}, None, model=tiny)
    z = {}
    for icp in (False, True):
        out = tmp_path / f"icp{int(icp)}"
        mv.process_multi_view_video(tmp_path / "subj" / "left.mp4", tmp_path / "subj" / "left.pt", tmp_path / "subj" / "right.mp4",
                                    tmp_path / "subj" / "right.pt", out, out / "inf", {"infer": {"gpu": 0, "icp": icp}},
                                    camera_head=head, steps_per_call=1)
        z[icp] = np.load(out / "inf" / "subj_multi_view_3d_info.npz")
    off, on = z[False], z[True]
    assert not bool(off["icp_refined"]) and bool(on["icp_refined"])
    assert np.array_equal(on["R"][:, 0], off["R"][:, 0]) and np.array_equal(on["t"][:, 0], off["t"][:, 0])
    assert np.array_equal(on["C"], off["C"]) and np.array_equal(on["camera_intrinsics"], off["camera_intrinsics"])
    for i in range(T):
        head.reconstruct_from_frames(i, [lf[i], rf[i]])
        wpd = head.last_world_points[0]
        res = geometry.icp_point_to_plane(wpd[0].reshape(-1, 3), wpd[1].reshape(-1, 3))
        R2, t2 = mv.apply_icp_update(off["R"][i], off["t"][i], res.transformation)
        assert np.array_equal(on["R"][i], R2) and np.array_equal(on["t"][i], t2)
        dev = torch.device("cuda", 0)
        x3d = geometry.triangulate_joints(torch.from_numpy(on["camera_intrinsics"][i][None]).to(dev, torch.float32),
                                          torch.from_numpy(R2[None]).to(dev, torch.float32),
                                          torch.from_numpy(t2[None]).to(dev, torch.float32),
                                          torch.from_numpy(np.stack([lk[i], rk[i]])[None]).to(dev, torch.float32))
        assert np.array_equal(on["x3d"][i], x3d[0].cpu().numpy())
        # ICP_with_bbox: the reference's signature on the same maps (boxes ignored)
        aligned, T_b = mv.ICP_with_bbox(wpd[0], wpd[1], lb[i], rb[i])
        assert np.array_equal(T_b, res.transformation) and aligned.shape == (wpd[0].numel() // 3, 3)
