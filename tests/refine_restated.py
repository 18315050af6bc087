"""Float64 NumPy restatement of the camera-and-points refinement (csrc/refine.hip; rules: DESIGN §2 "Camera + points
refinement").  One problem is one group: all V cameras of the group and its used points move together.  The statements
follow the kernel's, rule by rule; sums are NumPy's (the kernel's have a fixed order of their own: the two agree to
rounding, which rule 7's acceptance slack and rule 9's floor on the damping keep from growing into a different stopping
point).

Reference: VideoPose3D/slove_rt_from_3d.py --refine camera_points (x0 = pack(init, X) :236, the prior :159-161,
least_squares :244; X_opt :247 is computed and used for the errors :257-260 but not saved :263-271)."""
import numpy as np

from resect_restated import (LOSSES, MIN_POINTS, exp_coefficients, exp_so3, infer_K, ldl_solve, project, relative_pose,
                             residuals, weights_and_mask)

MAX_VIEWS = 4
TAU = 3e-8             # rule 8: stop on an accepted step with ||delta|| <= TAU (1 + ||(t, X)||)
LAMBDA_MIN = 1e-9      # rule 9: lambda >= LAMBDA_MIN max diag H of the current linearisation


# ---- rule 4 / 6: the linearisation ------------------------------------------------------------------------------------
def rho(r, loss, f_scale):
    """per residual component -> (rho' , the cost's summand before the factor 1/2 f^2 (soft_l1) or 1/2 (linear))"""
    if loss == "linear":
        return np.ones_like(r), r * r
    sq = np.sqrt(1.0 + (r / f_scale) * (r / f_scale))
    return 1.0 / sq, 2.0 * (sq - 1.0)


def linearise(K, R, t, X, X0, x, w, lambda_x, loss, f_scale):
    """K, R [V,3,3], t [V,3], X, X0 [n,3], x [V,n,2], w [V,n] -> dict(U [V,6,6], gc [V,6], Vp [n,3,3], gp [n,3],
    W [n,V,6,3], cost): the blocks of H = sum rho' J^T J and g = sum rho' J^T r over the cameras (U, gc), the points (Vp, gp)
    and between them (W)"""
    V, n = x.shape[:2]
    U, gc = np.zeros((V, 6, 6)), np.zeros((V, 6))
    Vp, gp, W = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros((n, V, 6, 3))
    half = 0.5 * (f_scale * f_scale) if loss == "soft_l1" else 0.5
    total = 0.0
    with np.errstate(all="ignore"):
        if lambda_x > 0:
            sl = np.sqrt(lambda_x)
            rp = sl * (X - X0)
            rho1, summand = rho(rp, loss, f_scale)
            total = total + summand.sum()
            Vp[:, [0, 1, 2], [0, 1, 2]] = rho1 * (sl * sl)
            gp += rho1 * (sl * rp)
        for v in range(V):
            q, z, uu, vv, r = residuals(K[v], R[v], t[v], X, x[v], w[v])
            fx, sk, fy = K[v, 0, 0], K[v, 0, 1], K[v, 1, 1]
            a = np.stack([np.stack([w[v] * (fx / z), w[v] * (sk / z), w[v] * (-(fx * uu + sk * vv) / z)], axis=1),
                          np.stack([np.zeros_like(z), w[v] * (fy / z), w[v] * (-(fy * vv) / z)], axis=1)], axis=1)  # [n,2,3]
            Jc = np.concatenate([np.cross(q[:, None, :], a), a], axis=2)                                          # [n,2,6]
            Jp = a @ R[v]                                                                                         # [n,2,3]
            rho1, summand = rho(r, loss, f_scale)
            total = total + summand.sum()
            U[v] = np.einsum("nc,nci,ncj->ij", rho1, Jc, Jc)
            gc[v] = np.einsum("nc,nci,nc->i", rho1, Jc, r)
            Vp += np.einsum("nc,nci,ncj->nij", rho1, Jp, Jp)
            gp += np.einsum("nc,nci,nc->ni", rho1, Jp, r)
            W[:, v] = np.einsum("nc,nci,ncj->nij", rho1, Jc, Jp)
    return dict(U=U, gc=gc, Vp=Vp, gp=gp, W=W, cost=half * total)


def max_diag(lin):
    return max(np.max(np.diagonal(lin["U"], axis1=1, axis2=2)), np.max(np.diagonal(lin["Vp"], axis1=1, axis2=2)))


def dense_system(lin):
    """-> (H [6V + 3n, 6V + 3n], g): cameras first, then the points"""
    U, W = lin["U"], lin["W"]
    V, n = U.shape[0], W.shape[0]
    m = 6 * V + 3 * n
    H, g = np.zeros((m, m)), np.zeros(m)
    for v in range(V):
        H[6 * v:6 * v + 6, 6 * v:6 * v + 6] = U[v]
        g[6 * v:6 * v + 6] = lin["gc"][v]
    for i in range(n):
        o = 6 * V + 3 * i
        H[o:o + 3, o:o + 3] = lin["Vp"][i]
        g[o:o + 3] = lin["gp"][i]
        for v in range(V):
            H[6 * v:6 * v + 6, o:o + 3] = W[i, v]
            H[o:o + 3, 6 * v:6 * v + 6] = W[i, v].T
    return H, g


# ---- rule 6: the step through the Schur complement on the points ---------------------------------------------------------
def solve3(Vs, b):
    """x with Vs x = b for symmetric Vs [n,3,3], b [n,...,3]: LDL^T without pivoting, as the kernel does it"""
    with np.errstate(all="ignore"):
        d0 = Vs[:, 0, 0]
        l10, l20 = Vs[:, 1, 0] / d0, Vs[:, 2, 0] / d0
        d1 = Vs[:, 1, 1] - l10 * l10 * d0
        l21 = (Vs[:, 2, 1] - l20 * l10 * d0) / d1
        d2 = Vs[:, 2, 2] - l20 * l20 * d0 - l21 * l21 * d1
        sh = (slice(None),) + (None,) * (b.ndim - 2)
        d0, d1, d2, l10, l20, l21 = (a[sh] for a in (d0, d1, d2, l10, l20, l21))
        y0 = b[..., 0]
        y1 = b[..., 1] - l10 * y0
        y2 = b[..., 2] - l20 * y0 - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = y0 / d0 - l10 * x1 - l20 * x2
    return np.stack([x0, x1, x2], axis=-1)


def schur_step(lin, lam):
    """(H + lam I) delta = -g, exactly: -> (dc [V,6], dX [n,3])"""
    U, gc, Vp, gp, W = (lin[k] for k in ("U", "gc", "Vp", "gp", "W"))
    V = U.shape[0]
    Vs = Vp + lam * np.eye(3)
    with np.errstate(all="ignore"):
        Y = solve3(Vs, W)                                          # [n,V,6,3]: rows W_iv[a] Vs^-1
        S = np.zeros((6 * V, 6 * V))
        rhs = np.zeros(6 * V)
        for v1 in range(V):
            for v2 in range(V):
                blk = -np.einsum("nak,nbk->ab", Y[:, v1], W[:, v2])
                if v1 == v2:
                    blk = (U[v1] + lam * np.eye(6)) + blk
                S[6 * v1:6 * v1 + 6, 6 * v2:6 * v2 + 6] = blk
            rhs[6 * v1:6 * v1 + 6] = -gc[v1] + np.einsum("nak,nk->a", Y[:, v1], gp)
        dc = ldl_solve(S, -rhs).reshape(V, 6)
        dX = -solve3(Vs, gp + np.einsum("nvak,va->nk", W, dc))
    return dc, dX


# ---- rule 7: the change of the cost, formed from the step -----------------------------------------------------------------
def cost_change(K, R, R1, t, X, X0, x, w, lambda_x, loss, f_scale, dc, dXe):
    """cost(Exp(om_v) R_v, t_v + dt_v, X + dXe) - cost(R, t, X); R1 = Exp(om) R; dXe = (X + dX) - X, the step X can take"""
    f2 = f_scale * f_scale

    def summed(r, dr):
        e = dr * (2.0 * r + dr)
        if loss == "linear":
            return e.sum()
        z0 = (r / f_scale) * (r / f_scale)
        dz = e / f2
        return (2.0 * dz / (np.sqrt(1.0 + (z0 + dz)) + np.sqrt(1.0 + z0))).sum()

    total = 0.0
    with np.errstate(all="ignore"):
        if lambda_x > 0:
            sl = np.sqrt(lambda_x)
            total = total + summed(sl * (X - X0), sl * dXe)
        for v in range(x.shape[0]):
            q, z, uu, vv, r = residuals(K[v], R[v], t[v], X, x[v], w[v])
            om = dc[v, :3]
            A, B = exp_coefficients(om)
            c1 = np.cross(om, q)
            d = ((A * c1 + B * np.cross(om, c1)) + dXe @ R1[v].T) + dc[v, 3:]
            z1 = z + d[:, 2]
            du, dv = (d[:, 0] - uu * d[:, 2]) / z1, (d[:, 1] - vv * d[:, 2]) / z1
            dr = np.stack([w[v] * (K[v, 0, 0] * du + K[v, 0, 1] * dv), w[v] * (K[v, 1, 1] * dv)], axis=1)
            total = total + summed(r, dr)
    return (0.5 * f2 if loss == "soft_l1" else 0.5) * total


# ---- rules 6 to 9: Levenberg-Marquardt --------------------------------------------------------------------------------------
def refine(K, R, t, X0, x, w, lambda_x, loss, f_scale, max_evals, tau=TAU, lambda_min=LAMBDA_MIN, Xs=None, trace=None):
    """-> dict(R, t, X, cost0, cost, n_evals, stopped); cost0 None: non-finite start.  Xs: the points' start when it is not
    X0 (the prior always pulls to X0)"""
    X = X0.copy() if Xs is None else Xs.copy()
    lin = linearise(K, R, t, X, X0, x, w, lambda_x, loss, f_scale)
    c = lin["cost"]
    out = dict(R=R, t=t, X=X, cost0=c, cost=c, n_evals=1, stopped=False)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(c)):
        out["cost0"] = None
        return out
    V = R.shape[0]
    lam = 1e-3 * max_diag(lin)
    while out["n_evals"] < max_evals:
        dc, dX = schur_step(lin, lam)
        with np.errstate(all="ignore"):
            Xn = X + dX
            dXe = Xn - X
            R1 = np.stack([exp_so3(dc[v, :3]) @ R[v] for v in range(V)])
            dcost = cost_change(K, R, R1, t, X, X0, x, w, lambda_x, loss, f_scale, dc, dXe)
        out["n_evals"] += 1
        if trace is not None:
            trace.append((lam, c, dcost, np.sqrt((dc * dc).sum() + (dXe * dXe).sum())))
        if np.isfinite(dcost) and dcost <= 1e-14 * c:          # c + dc <= c (1 + 1e-14)
            R, t, X = R1, t + dc[:, 3:], Xn
            lin = linearise(K, R, t, X, X0, x, w, lambda_x, loss, f_scale)
            c = lin["cost"]
            if not np.isfinite(c):
                break
            lam = max(lam / 10.0, lambda_min * max_diag(lin))
            if np.sqrt((dc * dc).sum() + (dXe * dXe).sum()) <= tau * (1.0 + np.sqrt((t * t).sum() + (X * X).sum())):
                out["stopped"] = True
                break
        else:
            lam = 10.0 * lam
            if not lam < 1e30:
                out["stopped"] = True
                break
    out.update(R=R, t=t, X=X, cost=c)
    return out


# ---- the whole call -----------------------------------------------------------------------------------------------------------
def refine_cameras_points(X, x2d, K=None, R0=None, t0=None, conf=None, group_size=None, lambda_x=0.0, loss="linear",
                          f_scale=1.0, min_conf=0.0, max_evals=200, groups=None, tau=TAU, lambda_min=LAMBDA_MIN, Xs=None):
    """X [N,3], x2d [V,N,2], K [V,3,3] | None, R0 [G,V,3,3], t0 [G,V,3] (required, as by the kernel), conf [V,N] | None ->
    dict of rule 10's outputs.  `groups`: compute these groups only (the others' entries stay NaN / 0, their X_opt X).  `Xs` [N,3]: the points start
    there and not at X, which stays the prior's centre (the kernel has no such argument: the sensitivity protocol's)."""
    X, x2d = np.asarray(X, np.float64), np.asarray(x2d, np.float64)
    V, N = x2d.shape[:2]
    gs = N if group_size is None else int(group_size)
    assert loss in LOSSES and gs >= 1 and N % gs == 0 and 1 <= V <= MAX_VIEWS
    G = N // gs
    R0, t0 = np.asarray(R0, np.float64), np.asarray(t0, np.float64)
    nan = lambda *s: np.full(s, np.nan)   # noqa: E731
    o = dict(R=nan(G, V, 3, 3), t=nan(G, V, 3), K=nan(G, V, 3, 3), X_opt=X.copy(), cost0=nan(G), cost=nan(G),
             n_evals=np.zeros(G, np.int32), n_points=np.zeros(G, np.int32), success=np.zeros(G, np.int32), err=nan(V, N),
             mean_err=nan(G, V), rms_err=nan(G, V), max_err=nan(G, V), moved=nan(G), R_rel=nan(G, V, 3, 3), t_rel=nan(G, V, 3))
    w_all, used_all = weights_and_mask(X, x2d, None if conf is None else np.asarray(conf, np.float64), min_conf)
    for gi in (range(G) if groups is None else groups):
        sl = slice(gi * gs, (gi + 1) * gs)
        used = used_all[sl]
        n = int(used.sum())
        o["n_points"][gi] = n
        if K is not None:
            o["K"][gi] = np.asarray(K, np.float64)
        if n < MIN_POINTS:
            continue
        Xu, xu, wu = X[sl][used], x2d[:, sl][:, used], w_all[:, sl][:, used]
        Kg = o["K"][gi] if K is not None else np.stack([infer_K(xu[v]) for v in range(V)])
        o["K"][gi] = Kg
        res = refine(Kg, R0[gi], t0[gi], Xu, xu, wu, float(lambda_x), loss, float(f_scale), int(max_evals), tau, lambda_min,
                     Xs=None if Xs is None else np.asarray(Xs, np.float64)[sl][used])
        if res["cost0"] is None:
            continue
        o["R"][gi], o["t"][gi] = res["R"], res["t"]
        idx = np.arange(gi * gs, (gi + 1) * gs)[used]
        o["X_opt"][idx] = res["X"]
        o["cost0"][gi], o["cost"][gi], o["n_evals"][gi], o["success"][gi] = res["cost0"], res["cost"], res["n_evals"], int(res["stopped"])
        for v in range(V):
            d = project(Kg[v], res["R"][v], res["t"][v], res["X"]) - xu[v]
            e = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            o["err"][v, idx] = e
            o["mean_err"][gi, v], o["rms_err"][gi, v], o["max_err"][gi, v] = e.sum() / n, np.sqrt((e * e).sum() / n), e.max()
        m = res["X"] - Xu
        o["moved"][gi] = np.sqrt((m * m).sum() / n)
        o["R_rel"][gi], o["t_rel"][gi] = relative_pose(o["R"][gi], o["t"][gi])
    return o
