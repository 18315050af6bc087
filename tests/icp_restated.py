"""Float64 restatement of the reference's ICP step (vggt/multi_view_process.py:427-520: Open3D's estimate_normals
and registration_icp with TransformationEstimationPointToPlane), as pinned by DESIGN §2 "ICP".  NumPy, with
scipy.spatial.cKDTree only to collect candidates: the decisions themselves use d^2 = dx*dx + dy*dy + dz*dz in
float64, the strict d^2 < r^2 test and the smaller-index tie rule.

The rules this build sets where Open3D depends on its implementation:
- a point is valid iff its coordinates are finite and x^2 + y^2 + z^2 > 1e-12 (the reference's ||p|| > 1e-6 lets
  inf points in; the two differ only on non-finite input);
- an equidistant correspondence goes to the target point with the smaller index;
- normals are float64 eigenvectors of the cumulant-form covariance ((0, 0, 1) below 3 neighbours), sign arbitrary.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

MIN_POINTS = 50   # multi_view_process.py:471-474


def valid_mask(P) -> np.ndarray:
    X = np.asarray(P, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1] + X[:, 2] * X[:, 2]
        return np.isfinite(X).all(axis=1) & (sq > 1e-12)


def _search_radius(r: float) -> float:
    return r * (1 + 1e-6) + 1e-12   # candidates only: the exact test follows


def normals(P, radius: float = 0.05):
    """valid points P [M, 3] (float32 values) -> (normals float64 [M, 3], neighbour counts [M])"""
    X = np.asarray(P, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    M = len(X)
    pairs = cKDTree(X).query_pairs(_search_radius(radius), output_type="ndarray")
    i, j = pairs[:, 0], pairs[:, 1]
    d = X[i] - X[j]
    keep = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] < radius * radius
    i, j = i[keep], j[keep]
    rows = np.concatenate([i, j, np.arange(M)])
    cols = np.concatenate([j, i, np.arange(M)])
    cnt = np.bincount(rows, minlength=M)
    Y = X[cols]
    s = np.stack([np.bincount(rows, Y[:, a], minlength=M) for a in range(3)], axis=1)
    ss = np.empty((M, 3, 3))
    for a in range(3):
        for b in range(a, 3):
            ss[:, a, b] = ss[:, b, a] = np.bincount(rows, Y[:, a] * Y[:, b], minlength=M)
    n = np.zeros((M, 3))
    n[:, 2] = 1.0
    ok = cnt >= 3
    if ok.any():
        m = s[ok] / cnt[ok, None]
        C = ss[ok] / cnt[ok, None, None] - m[:, :, None] * m[:, None, :]
        _, V = np.linalg.eigh(C)
        n[ok] = V[:, :, 0]
    return n, cnt


def transform(T, S) -> np.ndarray:
    """T s in float64 from the float32 source, summed left to right as the kernel does"""
    s = np.asarray(S, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    return np.stack([T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1] + T[r, 2] * s[:, 2] + T[r, 3] for r in range(3)], axis=1)


class Target:
    def __init__(self, P):
        self.X = np.asarray(P, dtype=np.float32).astype(np.float64).reshape(-1, 3)
        self.tree = cKDTree(self.X)

    def nearest(self, Y, max_dist: float):
        """-> (index into the target or -1, d^2) per query row"""
        M = len(self.X)
        k = min(8, M)
        _, idx = self.tree.query(Y, k=k, distance_upper_bound=_search_radius(max_dist))
        idx = idx.reshape(len(Y), k)
        have = idx < M
        c = np.where(have, idx, 0)
        d = Y[:, None, :] - self.X[c]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        d2 = np.where(have & (d2 < max_dist * max_dist), d2, np.inf)
        best = d2.min(axis=1)
        tie = (d2 == best[:, None]) & np.isfinite(d2)
        pick = np.where(tie, c, np.iinfo(np.int64).max).min(axis=1)
        found = np.isfinite(best)
        return np.where(found, pick, -1), np.where(found, best, 0.0)


def correspondences(src, tgt, T, max_dist: float = 0.05) -> np.ndarray:
    """original target index of every source point's correspondence (-1: none / invalid source point)"""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    vs, vt = valid_mask(src), valid_mask(tgt)
    out = np.full(len(src), -1, dtype=np.int64)
    if not vs.any() or not vt.any():
        return out
    ti = np.nonzero(vt)[0]
    c, _ = Target(tgt[vt]).nearest(transform(T, src[vs]), max_dist)
    out[np.nonzero(vs)[0]] = np.where(c >= 0, ti[np.maximum(c, 0)], -1)
    return out


def solve6_ldlt(JtJ: np.ndarray, Jtr: np.ndarray):
    """JtJ x = -Jtr by LDLT with diagonal pivoting (largest remaining diagonal first); a pivot of magnitude <= DBL_MIN
    contributes 0.  None if x is not finite."""
    A = [[float(JtJ[a, c]) for c in range(6)] for a in range(6)]
    b = [-float(v) for v in Jtr]
    perm = list(range(6))
    D = [0.0] * 6
    tiny = 2.2250738585072014e-308
    for j in range(6):
        piv = j
        for i in range(j + 1, 6):
            if abs(A[i][i]) > abs(A[piv][piv]):
                piv = i
        if piv != j:
            A[j], A[piv] = A[piv], A[j]
            for r in range(6):
                A[r][j], A[r][piv] = A[r][piv], A[r][j]
            perm[j], perm[piv] = perm[piv], perm[j]
        D[j] = A[j][j]
        for i in range(j + 1, 6):
            A[i][j] = A[i][j] / D[j] if abs(D[j]) > tiny else 0.0
        for i in range(j + 1, 6):
            for c in range(j + 1, i + 1):
                A[i][c] -= A[i][j] * D[j] * A[c][j]
                A[c][i] = A[i][c]
    y = [b[perm[i]] for i in range(6)]
    for i in range(6):
        for c in range(i):
            y[i] -= A[i][c] * y[c]
    for i in range(6):
        y[i] = y[i] / D[i] if abs(D[i]) > tiny else 0.0
    for i in range(5, -1, -1):
        for c in range(i + 1, 6):
            y[i] -= A[c][i] * y[c]
    x = np.zeros(6)
    for i in range(6):
        x[perm[i]] = y[i]
    return x if np.isfinite(x).all() else None


def euler_to_mat(x) -> np.ndarray:
    """x [6] -> 4x4: R = Rz(x2) Ry(x1) Rx(x0), translation x3..5 (Open3D's TransformVector6dToMatrix4d)"""
    a, b, g = x[0], x[1], x[2]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    U = np.eye(4)
    U[:3, :3] = Rz @ (Ry @ Rx)
    U[:3, 3] = x[3:6]
    return U


def mat_to_euler(U) -> np.ndarray:
    """inverse of euler_to_mat for |x1| < pi / 2"""
    R = np.asarray(U)[:3, :3]
    return np.array([np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(R[2, 0]), np.arctan2(R[1, 0], R[0, 0]), *np.asarray(U)[:3, 3]])


def icp_point_to_plane(src, tgt, max_correspondence_distance=0.05, normal_radius=0.05, max_iteration=200,
                       relative_fitness=1e-6, relative_rmse=1e-6, init=None):
    """-> (T float64 [4, 4], fitness, inlier_rmse, iterations)"""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    S, P = src[valid_mask(src)], tgt[valid_mask(tgt)]
    if len(S) < MIN_POINTS or len(P) < MIN_POINTS:
        return np.eye(4), 0.0, 0.0, 0
    N, _ = normals(P, normal_radius)
    tg = Target(P)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)

    def evaluate(T):
        Y = transform(T, S)
        c, d2 = tg.nearest(Y, max_correspondence_distance)
        m = c >= 0
        y, t, n = Y[m], tg.X[c[m]], N[c[m]]
        r = (y[:, 0] - t[:, 0]) * n[:, 0] + (y[:, 1] - t[:, 1]) * n[:, 1] + (y[:, 2] - t[:, 2]) * n[:, 2]
        J = np.stack([y[:, 1] * n[:, 2] - y[:, 2] * n[:, 1], y[:, 2] * n[:, 0] - y[:, 0] * n[:, 2],
                      y[:, 0] * n[:, 1] - y[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
        cnt = int(m.sum())
        fit = cnt / len(S)
        rmse = float(np.sqrt(d2[m].sum() / cnt)) if cnt else 0.0
        return J.T @ J, J.T @ r, cnt, fit, rmse

    JtJ, Jtr, cnt, fit, rmse = evaluate(T)
    it = 0
    while it < max_iteration:
        x = solve6_ldlt(JtJ, Jtr) if cnt > 0 else None
        U = euler_to_mat(x) if x is not None else np.eye(4)
        T = U @ T
        it += 1
        fit0, rmse0 = fit, rmse
        JtJ, Jtr, cnt, fit, rmse = evaluate(T)
        if abs(fit0 - fit) < relative_fitness and abs(rmse0 - rmse) < relative_rmse:
            break
    return T, fit, rmse, it
