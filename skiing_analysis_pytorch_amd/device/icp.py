"""Point-to-plane ICP (csrc/icp.hip; C-ABI: skimi_estimate_normals, skimi_icp_correspondences, skimi_icp_point_to_plane):
Open3D's estimate_normals + registration_icp restated, vggt/multi_view_process.py:427-520; DESIGN §2 "ICP".

Rules where Open3D's result depends on its implementation: a point is valid iff its coordinates are finite and
x^2 + y^2 + z^2 > 1e-12 (the reference keeps ||p|| > 1e-6, which lets inf points in: the two differ only on
non-finite input); neighbours / correspondences lie at d^2 < r^2 in float64; a tie between equidistant target points
goes to the smaller index; every sum has a fixed order (bitwise reproducible); normals are float64 eigenvectors
solved to convergence (Jacobi), their sign arbitrary.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from .._args import contig_as, f64, host_f64, i32, on_device, workspace
from .._lib import SkimiError, check, current_stream, lib, ptr


def _cloud(points: torch.Tensor, what: str) -> torch.Tensor:
    on_device(what, points, what="a device tensor")
    if points.shape[-1] != 3:
        raise SkimiError(f"{what}: points must be [..., 3], got {tuple(points.shape)}")
    return contig_as(points.reshape(-1, 3))


def _icp_workspace(n_src: int, n_tgt: int, device) -> torch.Tensor:
    return workspace(device, lib().skimi_icp_workspace_bytes(n_src, n_tgt))


def _mat4(T) -> "C.Array":
    return (C.c_double * 16)(*host_f64(T).reshape(4, 4).ravel().tolist())


def estimate_normals(points: torch.Tensor, radius: float = 0.05):
    """Radius normals (estimate_normals(KDTreeSearchParamRadius(radius)), multi_view_process.py:487-496) of a device
    cloud [..., 3] -> (normals float64 [N, 3], neighbour counts int32 [N]).  Neighbours are the valid points at
    d < radius, the point itself included; with >= 3 of them the normal is the smallest-eigenvalue eigenvector of their
    covariance, else (0, 0, 1).  Invalid points get (0, 0, 0) and 0."""
    p = _cloud(points, "estimate_normals")
    n = p.shape[0]
    normals, counts = f64(p.device, n, 3), i32(p.device, n)
    ws = _icp_workspace(0, n, p.device)
    check(lib().skimi_estimate_normals(ptr(p), n, float(radius), ptr(normals), ptr(counts), ptr(ws), ws.numel(),
                                       current_stream()), "skimi_estimate_normals")
    return normals, counts


def icp_correspondences(source: torch.Tensor, target: torch.Tensor, transformation=None, max_distance: float = 0.05):
    """Index of the nearest valid target point at d < max_distance of every source point under `transformation`
    (4x4, default identity) -> int64 [N_src] device tensor, -1 = no correspondence (or invalid source point).
    Ties go to the smaller target index."""
    s, t = _cloud(source, "icp_correspondences"), _cloud(target, "icp_correspondences")
    out = i32(s.device, s.shape[0])
    ws = _icp_workspace(s.shape[0], t.shape[0], s.device)
    T = _mat4(np.eye(4) if transformation is None else transformation)
    check(lib().skimi_icp_correspondences(ptr(s), s.shape[0], ptr(t), t.shape[0], T, float(max_distance), ptr(out), ptr(ws),
                                          ws.numel(), current_stream()), "skimi_icp_correspondences")
    return out.to(torch.int64)


@dataclass
class ICPResult:
    """The fields of Open3D's RegistrationResult that the reference reads (transformation) or reports."""
    transformation: np.ndarray   # float64 [4, 4]
    fitness: float               # correspondences / valid source points, last evaluation
    inlier_rmse: float           # sqrt(sum d^2 / correspondences), last evaluation
    iterations: int              # updates applied


def icp_point_to_plane(source: torch.Tensor, target: torch.Tensor, max_correspondence_distance: float = 0.05,
                       normal_radius: float = 0.05, max_iteration: int = 200, relative_fitness: float = 1e-6,
                       relative_rmse: float = 1e-6, init=None) -> ICPResult:
    """registration_icp(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) on device clouds [..., 3], target normals
    from estimate_normals(normal_radius) (multi_view_process.py:487-505).  Fewer than 50 valid points in either cloud:
    identity and 0 iterations (:471-474)."""
    s, t = _cloud(source, "icp_point_to_plane"), _cloud(target, "icp_point_to_plane")
    ws = _icp_workspace(s.shape[0], t.shape[0], s.device)
    T_out = (C.c_double * 16)()
    fit, rmse, iters = C.c_double(), C.c_double(), C.c_int32()
    check(lib().skimi_icp_point_to_plane(ptr(s), s.shape[0], ptr(t), t.shape[0], float(max_correspondence_distance),
                                         float(normal_radius), int(max_iteration), float(relative_fitness), float(relative_rmse),
                                         None if init is None else _mat4(init), T_out, C.byref(fit), C.byref(rmse),
                                         C.byref(iters), ptr(ws), ws.numel(), current_stream()), "skimi_icp_point_to_plane")
    return ICPResult(np.array(T_out[:], dtype=np.float64).reshape(4, 4), fit.value, rmse.value, iters.value)
