"""CPU: the float64 restatement of the reference's ICP (tests/icp_restated.py) is point-to-plane ICP, and the
host-side pieces of the multi-view ICP step (the Euler convention, the camera update of
vggt/multi_view_process.py:271-275, the device-only rule of geometry.icp_point_to_plane)."""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import icp_restated as ref
from skiing_analysis_pytorch_amd import _lib, geometry
from skiing_analysis_pytorch_amd import multi_view_process as mv


def _motion(deg, axis, trans):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.deg2rad(deg) * np.asarray(axis, float) / np.linalg.norm(axis)).as_matrix()
    T[:3, 3] = trans
    return T


def _wavy(n=90, spacing=0.011, seed=0):
    rng = np.random.default_rng(seed)
    u = (np.arange(n) - n / 2) * spacing
    x, y = np.meshgrid(u, u, indexing="ij")
    x = x + rng.uniform(-0.3, 0.3, x.shape) * spacing
    y = y + rng.uniform(-0.3, 0.3, y.shape) * spacing
    z = 0.12 * np.sin(3.1 * x + 0.4) * np.cos(2.3 * y) + 0.08 * x * y
    return np.stack([x, y, z + 1.0], -1).reshape(-1, 3).astype(np.float32)


def test_normals_of_plane_and_sphere_cap():
    rng = np.random.default_rng(1)
    # a tilted plane n . p = 0.7
    n_true = np.array([0.3, -0.5, 0.8])
    n_true /= np.linalg.norm(n_true)
    a = np.cross(n_true, [1, 0, 0])
    a /= np.linalg.norm(a)
    b = np.cross(n_true, a)
    uv = rng.uniform(-0.4, 0.4, (4000, 2))
    P = (0.7 * n_true + uv[:, :1] * a + uv[:, 1:] * b).astype(np.float32)
    n, cnt = ref.normals(P, 0.05)
    assert cnt.min() >= 10
    assert np.abs(np.abs(n @ n_true) - 1).max() < 1e-9
    # a sphere cap of radius 2: the normal at p is p / |p| (the neighbourhood is symmetric only up to sampling,
    # so the test uses points whose neighbourhood is a full, dense ring of the lattice below)
    th = np.deg2rad(np.linspace(0, 12, 120))
    ph = np.linspace(0, 2 * np.pi, 900, endpoint=False)
    T_, P_ = np.meshgrid(th, ph, indexing="ij")
    S = np.stack([np.sin(T_) * np.cos(P_), np.sin(T_) * np.sin(P_), np.cos(T_)], -1).reshape(-1, 3) * 2.0
    S = S.astype(np.float32)
    n, cnt = ref.normals(S, 0.05)
    apex = np.nonzero(np.linalg.norm(S[:, :2], axis=1) < 1e-6)[0]
    assert len(apex) and (cnt[apex] >= 3).all()
    assert np.abs(np.abs(n[apex] @ np.array([0, 0, 1.0])) - 1).max() < 1e-9
    # the apex neighbourhood is rotationally symmetric: exact; elsewhere the covariance of a curved patch has its
    # smallest axis along the local normal up to O(r^2 / R^2) -- check the ring rows whose neighbourhoods are complete
    inner = np.nonzero((T_.reshape(-1) > np.deg2rad(3)) & (T_.reshape(-1) < np.deg2rad(9)))[0]
    radial = S[inner] / np.linalg.norm(S[inner], axis=1, keepdims=True)
    assert np.abs(np.abs(np.einsum("ij,ij->i", n[inner], radial)) - 1).max() < 1e-4
    # isolated points and pairs: (0, 0, 1)
    iso = np.array([[5, 5, 5], [-5, 5, 5], [-5, -5, 5], [-5, -5, 5.01]], np.float32)
    n, cnt = ref.normals(iso, 0.05)
    assert list(cnt) == [1, 1, 2, 2]
    assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (4, 1)))


def test_normals_cumulant_form_matches_eigh_of_centered_covariance():
    P = _wavy(40)
    n, cnt = ref.normals(P, 0.05)
    X = P.astype(np.float64)
    for i in (0, 77, 500, 1599):
        d = X - X[i]
        nb = X[(d * d).sum(1) < 0.0025]
        assert len(nb) == cnt[i]
        w, V = np.linalg.eigh(np.cov(nb.T, bias=True))
        assert abs(abs(V[:, 0] @ n[i]) - 1) < 1e-9


def test_restatement_recovers_a_known_motion():
    tgt = _wavy()
    for deg, axis, trans in ((2.0, (0.3, 1, 0.2), (0.01, -0.005, 0.004)), (1.2, (1, -0.4, 0.7), (-0.006, 0.008, 0.0))):
        M = _motion(deg, axis, trans)
        Minv = np.linalg.inv(M)
        src = (tgt.astype(np.float64) @ Minv[:3, :3].T + Minv[:3, 3]).astype(np.float32)
        T, fit, rmse, it = ref.icp_point_to_plane(src, tgt)
        assert np.abs(T - M).max() < 1e-6, (np.abs(T - M).max(), it)
        assert fit > 0.97 and rmse < 1e-6 and 1 < it < 200


def test_fewer_than_50_valid_points_is_identity():
    P = _wavy(7)                                            # 49 points
    bad = np.array([[0, 0, 0], [np.nan, 1, 1], [np.inf, 0, 0], [1e-7, 0, 0]], np.float32)
    T, fit, rmse, it = ref.icp_point_to_plane(np.concatenate([P, bad]), _wavy(30))
    assert np.array_equal(T, np.eye(4)) and it == 0 and fit == 0 and rmse == 0
    assert ref.valid_mask(bad).tolist() == [False, False, False, False]


def test_euler_convention_round_trips():
    rng = np.random.default_rng(3)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-1.2, 1.2, 3), rng.normal(size=3)])
        U = ref.euler_to_mat(x)
        assert np.allclose(ref.mat_to_euler(U), x, atol=1e-12, rtol=0)
        # R = Rz(x2) Ry(x1) Rx(x0): intrinsic z-y'-x'' with angles (x2, x1, x0)
        assert np.allclose(U[:3, :3], Rotation.from_euler("ZYX", [x[2], x[1], x[0]]).as_matrix(), atol=1e-14)
        assert np.allclose(U[:3, 3], x[3:]) and np.array_equal(U[3], [0, 0, 0, 1])


def test_ldlt_solve_matches_numpy():
    rng = np.random.default_rng(5)
    for _ in range(10):
        J = rng.normal(size=(40, 6))
        r = rng.normal(size=40)
        x = ref.solve6_ldlt(J.T @ J, J.T @ r)
        assert np.allclose(x, np.linalg.solve(J.T @ J, -(J.T @ r)), rtol=1e-10, atol=1e-12)


def test_camera_update_reproduces_reference_lines():
    """multi_view_process.py:271-275 on fixed matrices"""
    R = np.stack([Rotation.from_euler("xyz", [0.1, -0.2, 0.3]).as_matrix(), Rotation.from_euler("xyz", [-0.4, 0.25, 1.1]).as_matrix()])
    t = np.array([[0.5, -1.0, 2.0], [1.5, 0.25, -3.0]])
    T = _motion(1.7, (0.2, 0.9, -0.1), (0.03, -0.02, 0.01))
    R2, t2 = mv.apply_icp_update(R, t, T)
    R_update, t_update = T[:3, :3], T[:3, 3]
    want_R1 = R_update @ R[1]
    want_t1 = R_update @ t[1] + t_update
    assert np.array_equal(R2[0], R[0]) and np.array_equal(t2[0], t[0])
    assert np.array_equal(R2[1], want_R1) and np.array_equal(t2[1], want_t1)
    assert not np.array_equal(R2[1], R[1])       # the inputs are copied, not updated in place
    assert np.array_equal(mv.apply_icp_update(R, t, np.eye(4))[1], t)


def test_icp_entry_points_reject_host_tensors():
    P = torch.from_numpy(_wavy(10))
    for call in (lambda: geometry.icp_point_to_plane(P, P), lambda: geometry.estimate_normals(P),
                 lambda: geometry.icp_correspondences(P, P)):
        with pytest.raises(_lib.SkimiError, match="device tensor"):
            call()


def test_icp_workspace_grows_with_the_clouds():
    lib = _lib.lib()
    small, big = lib.skimi_icp_workspace_bytes(1000, 1000), lib.skimi_icp_workspace_bytes(268324, 268324)
    assert 0 < small < big
    assert lib.skimi_icp_workspace_bytes(0, 1000) <= small
    assert lib.skimi_icp_point_to_plane(None, 0, None, 0, 0.05, 0.05, 200, 1e-6, 1e-6, None, None, None, None, None, None, 0,
                                        None) != 0
    assert b"bad arguments" in lib.skimi_last_error()
