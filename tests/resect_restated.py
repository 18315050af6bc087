"""Float64 NumPy restatement of the camera resection (csrc/resect.hip; rules: DESIGN §2 "Resection").  One problem is one
(group, view) pair; the problems are independent.  The statements follow the kernel's, rule by rule; sums are NumPy's
(the kernel's have a fixed order of their own: the two agree to rounding, which rule 5's acceptance slack keeps from
growing into a different stopping point).

Reference: VideoPose3D/slove_rt_from_3d.py (mask :97-101, weights :88-95, K :65-73, residuals :140-168, least_squares
:244, relative pose :252-254)."""
import numpy as np

MIN_POINTS = 6
SMALL_ANGLE2 = 1e-8
LOSSES = ("linear", "soft_l1")


# ---- rule 1 -----------------------------------------------------------------------------------------------------------
def weights_and_mask(X, x2d, conf, min_conf):
    """X [N,3], x2d [V,N,2], conf [V,N] | None -> (w [V,N], used [N])"""
    V, N = x2d.shape[:2]
    used = np.isfinite(X).all(axis=1) & np.isfinite(x2d).all(axis=(0, 2))
    if conf is None:
        return np.ones((V, N)), used
    w = np.where(np.isfinite(conf), conf, 0.0)
    w = np.minimum(np.maximum(w, 0.0), 1.0)
    return w, used & (w >= min_conf).all(axis=0)


# ---- rule 2 -----------------------------------------------------------------------------------------------------------
def infer_K(x):
    n = x.shape[0]
    c = x.sum(axis=0) / n
    s = np.sqrt(((x - c) ** 2).sum(axis=0) / n)
    f = 2.0 * max(s[0] + 1e-6, s[1] + 1e-6)
    return np.array([[f, 0.0, c[0]], [0.0, f, c[1]], [0.0, 0.0, 1.0]])


# ---- rule 3 -----------------------------------------------------------------------------------------------------------
def jacobi(M, max_sweeps=60):
    """cyclic Jacobi of a symmetric n x n to convergence -> (diagonal, eigenvectors in columns)"""
    M = M.copy()
    n = M.shape[0]
    Q = np.eye(n)
    iu = np.triu_indices(n, 1)
    for _ in range(max_sweeps):
        off = (M[iu] ** 2).sum()
        diag = (np.diag(M) ** 2).sum()
        if not np.isfinite(off) or off <= 1e-40 * diag or off == 0.0:
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                if M[p, q] == 0.0:
                    continue
                with np.errstate(over="ignore"):
                    theta = (M[q, q] - M[p, p]) / (2.0 * M[p, q])
                    tn = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(tn * tn + 1.0)
                sn = tn * cs
                mp, mq = M[:, p].copy(), M[:, q].copy()
                M[:, p] = cs * mp - sn * mq
                M[:, q] = sn * mp + cs * mq
                mp, mq = M[p, :].copy(), M[q, :].copy()
                M[p, :] = cs * mp - sn * mq
                M[q, :] = sn * mp + cs * mq
                M[p, q] = M[q, p] = 0.0
                qp, qq = Q[:, p].copy(), Q[:, q].copy()
                Q[:, p] = cs * qp - sn * qq
                Q[:, q] = sn * qp + cs * qq
    return np.diag(M).copy(), Q


def normalised_rays(K, x):
    v = (x[:, 1] - K[1, 2]) / K[1, 1]
    u = (x[:, 0] - K[0, 2] - K[0, 1] * v) / K[0, 0]
    return u, v


def dlt_init(K, X, x):
    """DLT resection of the used points X [n,3], x [n,2] -> (R, t); non-finite where the system is degenerate"""
    n = X.shape[0]
    u, v = normalised_rays(K, x)
    c = X.sum(axis=0) / n
    d = X - c
    s = np.sqrt(3.0) / (np.sqrt((d * d).sum(axis=1)).sum() / n)
    Xh = np.concatenate([s * d, np.ones((n, 1))], axis=1)
    S = [np.einsum("n,na,nb->ab", wk, Xh, Xh) for wk in (np.ones(n), u, v, u * u + v * v)]
    A = np.zeros((12, 12))
    A[0:4, 0:4] = S[0]
    A[4:8, 4:8] = S[0]
    A[0:4, 8:12] = A[8:12, 0:4] = -S[1]
    A[4:8, 8:12] = A[8:12, 4:8] = -S[2]
    A[8:12, 8:12] = S[3]
    lam, Q = jacobi(A)
    P = Q[:, int(np.argmin(lam))].reshape(3, 4)
    M = P[:, :3]
    det = (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
           + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    if det < 0:
        P = -P
        M = P[:, :3]
    lam3, W = jacobi(M.T @ M)
    with np.errstate(all="ignore"):
        sig = np.sqrt(np.maximum(lam3, 0.0))
        R = M @ (W * (1.0 / sig)) @ W.T          # U V^T of M = U S V^T
        tn = P[:, 3] * 3.0 / (sig[0] + sig[1] + sig[2])
        t = tn / s - R @ c
    return R, t


# ---- rules 4 and 5 ----------------------------------------------------------------------------------------------------
def exp_so3(w):
    """rodrigues.h's Rodrigues with the Taylor branch"""
    A, B = exp_coefficients(w)
    Kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + A * Kx + B * (Kx @ Kx)


def project(K, R, t, X):
    Xc = X @ R.T + t
    with np.errstate(all="ignore"):
        u, v = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    return np.stack([K[0, 0] * u + K[0, 1] * v + K[0, 2], K[1, 1] * v + K[1, 2]], axis=1)


def residuals(K, R, t, X, x, w):
    """-> q = R X, z, u, v, r [n,2] = w ((fx u + sk v) + (cx - x), fy v + (cy - y)): the principal point is folded into the
    keypoint, so that what is rounded last is the offset from it, not the ~1000 px coordinate"""
    q = X @ R.T
    Xc = q + t
    z = Xc[:, 2]
    u, v = Xc[:, 0] / z, Xc[:, 1] / z
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    r = np.stack([w * ((fx * u + sk * v) + (cx - x[:, 0])), w * (fy * v + (cy - x[:, 1]))], axis=1)
    return q, z, u, v, r


def normal_equations(K, R, t, X, x, w, loss, f_scale):
    """-> (H [6,6], g [6], cost) at (R, t)"""
    with np.errstate(all="ignore"):
        q, z, u, v, r = residuals(K, R, t, X, x, w)
        fx, sk, fy = K[0, 0], K[0, 1], K[1, 1]
        a = np.stack([np.stack([w * (fx / z), w * (sk / z), w * (-(fx * u + sk * v) / z)], axis=1),
                      np.stack([np.zeros_like(z), w * (fy / z), w * (-(fy * v) / z)], axis=1)], axis=1)  # [n,2,3]
        J = np.concatenate([np.cross(q[:, None, :], a), a], axis=2)                                      # [n,2,6]
        if loss == "linear":
            rho1 = np.ones_like(r)
            cost = 0.5 * (r * r).sum()
        else:
            zz = (r / f_scale) ** 2
            sq = np.sqrt(1.0 + zz)
            rho1 = 1.0 / sq
            cost = 0.5 * (f_scale * f_scale) * (2.0 * (sq - 1.0)).sum()
        H = np.einsum("nc,nci,ncj->ij", rho1, J, J)
        g = np.einsum("nc,nci,nc->i", rho1, J, r)
    return H, g, cost


def exp_coefficients(w):
    """A = sin(th)/th, B = (1 - cos(th))/th^2 of rodrigues.h's Rodrigues, with its Taylor branch"""
    s = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if s < SMALL_ANGLE2:
        return 1.0 - s / 6.0 + s * s / 120.0, 0.5 - s / 24.0 + s * s / 720.0
    th = np.sqrt(s)
    return np.sin(th) / th, (1.0 - np.cos(th)) / s


def cost_change(K, R, t, X, x, w, loss, f_scale, d):
    """cost(Exp(d[:3]) R, t + d[3:]) - cost(R, t), formed from the step: the change of the camera point is
    dX = A (om x q) + B om x (om x q) + dt, of the ray du = (dX - u dZ) / (Z + dZ), of a residual dr = w (fx du + sk dv),
    and of its square dr (2 r + dr).  Every term is as accurate as the step is small, where the difference of two
    rounded costs carries the rounding of both (~3e-14 relative at 17 points, K ~ 1100 px, 1 px residuals)."""
    with np.errstate(all="ignore"):
        q, z, u, v, r = residuals(K, R, t, X, x, w)
        om = d[:3]
        A, B = exp_coefficients(om)
        c1 = np.cross(om, q)
        dX = A * c1 + B * np.cross(om, c1) + d[3:]
        z1 = z + dX[:, 2]
        du, dv = (dX[:, 0] - u * dX[:, 2]) / z1, (dX[:, 1] - v * dX[:, 2]) / z1
        dr = np.stack([w * (K[0, 0] * du + K[0, 1] * dv), w * (K[1, 1] * dv)], axis=1)
        e = dr * (2.0 * r + dr)
        if loss == "linear":
            return 0.5 * e.sum()
        f2 = f_scale * f_scale
        z0 = (r / f_scale) ** 2
        dz = e / f2
        return 0.5 * f2 * (2.0 * dz / (np.sqrt(1.0 + (z0 + dz)) + np.sqrt(1.0 + z0))).sum()


def ldl_solve(H, g):
    """x with H x = -g by LDL^T without pivoting"""
    n = H.shape[0]
    L, D = np.eye(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            D[j] = H[j, j] - sum(L[j, k] * L[j, k] * D[k] for k in range(j))
            for i in range(j + 1, n):
                L[i, j] = (H[i, j] - sum(L[i, k] * L[j, k] * D[k] for k in range(j))) / D[j]
        y = np.zeros(n)
        for i in range(n):
            y[i] = -g[i] - sum(L[i, k] * y[k] for k in range(i))
        y = y / D
        x = np.zeros(n)
        for i in reversed(range(n)):
            x[i] = y[i] - sum(L[k, i] * x[k] for k in range(i + 1, n))
    return x


def refine(K, R, t, X, x, w, loss, f_scale, max_evals):
    """Levenberg-Marquardt of rule 5 -> dict(R, t, cost0, cost, n_evals, stopped); cost0 None: non-finite start"""
    H, g, c = normal_equations(K, R, t, X, x, w, loss, f_scale)
    out = dict(R=R, t=t, cost0=c, cost=c, n_evals=1, stopped=False)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(c)):
        out["cost0"] = None
        return out
    lam = 1e-3 * max(H[i, i] for i in range(6))
    while out["n_evals"] < max_evals:
        d = ldl_solve(H + lam * np.eye(6), g)
        dc = cost_change(K, R, t, X, x, w, loss, f_scale, d)
        out["n_evals"] += 1
        if np.isfinite(dc) and dc <= 1e-14 * c:          # c + dc <= c (1 + 1e-14)
            R, t = exp_so3(d[:3]) @ R, t + d[3:]
            H, g, c = normal_equations(K, R, t, X, x, w, loss, f_scale)
            if not np.isfinite(c):
                break
            lam = lam / 10.0
            if np.sqrt((d * d).sum()) <= 1e-14 * (1.0 + np.sqrt((t * t).sum())):
                out["stopped"] = True
                break
        else:
            lam = 10.0 * lam
            if not lam < 1e30:
                out["stopped"] = True
                break
    out.update(R=R, t=t, cost=c)
    return out


# ---- the whole call ---------------------------------------------------------------------------------------------------
def resect_cameras(X, x2d, K=None, conf=None, group_size=None, R0=None, t0=None, loss="linear", f_scale=1.0, min_conf=0.0,
                   max_evals=200, groups=None):
    """X [N,3], x2d [V,N,2], K [V,3,3] | None, conf [V,N] | None, R0 [G,V,3,3], t0 [G,V,3] | None -> dict of rule 6's
    outputs.  `groups`: compute these groups only (the others' entries stay NaN / 0)."""
    X, x2d = np.asarray(X, np.float64), np.asarray(x2d, np.float64)
    V, N = x2d.shape[:2]
    gs = N if group_size is None else int(group_size)
    assert loss in LOSSES and gs >= 1 and N % gs == 0
    G = N // gs
    nan = lambda *s: np.full(s, np.nan)   # noqa: E731
    o = dict(R=nan(G, V, 3, 3), t=nan(G, V, 3), K=nan(G, V, 3, 3), cost0=nan(G, V), cost=nan(G, V),
             n_evals=np.zeros((G, V), np.int32), n_points=np.zeros((G, V), np.int32), success=np.zeros((G, V), np.int32),
             err=nan(V, N), mean_err=nan(G, V), rms_err=nan(G, V), max_err=nan(G, V), R_rel=nan(G, V, 3, 3), t_rel=nan(G, V, 3))
    w_all, used_all = weights_and_mask(X, x2d, None if conf is None else np.asarray(conf, np.float64), min_conf)
    for gi in (range(G) if groups is None else groups):
        sl = slice(gi * gs, (gi + 1) * gs)
        used = used_all[sl]
        n = int(used.sum())
        for v in range(V):
            o["n_points"][gi, v] = n
            if K is not None:
                o["K"][gi, v] = np.asarray(K, np.float64)[v]
            if n < MIN_POINTS:
                continue
            Xu, xu, wu = X[sl][used], x2d[v, sl][used], w_all[v, sl][used]
            Kv = o["K"][gi, v] if K is not None else infer_K(xu)
            o["K"][gi, v] = Kv
            if R0 is not None:
                Ri, ti = np.asarray(R0, np.float64)[gi, v], np.asarray(t0, np.float64)[gi, v]
            else:
                Ri, ti = dlt_init(Kv, Xu, xu)
            res = refine(Kv, Ri, ti, Xu, xu, wu, loss, float(f_scale), int(max_evals))
            if res["cost0"] is None:
                continue
            o["R"][gi, v], o["t"][gi, v] = res["R"], res["t"]
            o["cost0"][gi, v], o["cost"][gi, v], o["n_evals"][gi, v] = res["cost0"], res["cost"], res["n_evals"]
            o["success"][gi, v] = int(res["stopped"])
            d = project(Kv, res["R"], res["t"], Xu) - xu
            e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            err = nan(gs)
            err[used] = e
            o["err"][v, sl] = err
            o["mean_err"][gi, v], o["rms_err"][gi, v], o["max_err"][gi, v] = e.sum() / n, np.sqrt((e * e).sum() / n), e.max()
        o["R_rel"][gi], o["t_rel"][gi] = relative_pose(o["R"][gi], o["t"][gi])
    return o


def relative_pose(R, t):
    """R, t [V,...] -> R_rel = R_v R_0^T, t_rel = t_v - R_rel t_0 (:252-254)"""
    R_rel = np.stack([Rv @ R[0].T for Rv in R])
    return R_rel, np.stack([tv - Rr @ t[0] for tv, Rr in zip(t, R_rel)])
