"""NumPy float64 restatement of the camera calibration (DESIGN §2 "Calibration"; csrc/calibrate.hip), rule by rule.  The
homographies are tests/bev_restated.py's, the lens model is tests/lens_restated.py's (rule 2 of the lens block), Exp is
tests/resect_restated.py's.  The sums are NumPy's, not the kernel's butterfly: the two agree to rounding, not to the bit.

Parameters: 12 intrinsics fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 (bit i of free_mask frees parameter i), then per used view
(w, dt) with R <- Exp(w) R, t <- t + dt."""
import numpy as np

import bev_restated as bv
import lens_restated as lr
import resect_restated as rr

NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")
NI = 12
TAU, LAM0, LAM_MIN, LAM_MAX = 3e-8, 1e-3, 1e-16, 1e30


def free_mask(rational_model=True, zero_tangent=False, names=None):
    """the reference's switches, or an explicit tuple of names -> the 12-bit mask"""
    if names is None:
        names = ["fx", "fy", "cx", "cy", "k1", "k2", "k3"] + (["k4", "k5", "k6"] if rational_model else [])
        names += [] if zero_tangent else ["p1", "p2"]
    return sum(1 << NAMES.index(k) for k in set(names))


def dist12(p):
    """the 12 parameters -> the lens block's dist [12]"""
    return np.concatenate([p[4:12], np.zeros(4)])


# ---- rule 4 -------------------------------------------------------------------------------------------------------------
def project(p, R, t, obj):
    """-> pixels [n, 2] of the board's corners obj [n, 2] at z = 0"""
    q = obj @ R[:, :2].T
    Xc = q + t
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    xd, yd = lr.distort_normalized(x, y, dist12(p))
    return np.stack([p[0] * xd + p[2], p[1] * yd + p[3]], -1)


def jacobians(p, R, t, obj, mask):
    """analytic Jacobians of the pixel: Ji [n, 2, 12] over the intrinsics (fixed columns zero), Jp [n, 2, 6] over (w, dt)"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = p
    q = obj @ R[:, :2].T
    z = q[:, 2] + t[2]
    x, y = (q[:, 0] + t[0]) / z, (q[:, 1] + t[1]) / z
    r2 = x * x + y * y
    r4, r6 = r2 * r2, r2 * r2 * r2
    num, den = 1.0 + k1 * r2 + k2 * r4 + k3 * r6, 1.0 + k4 * r2 + k5 * r4 + k6 * r6
    c, a = num / den, 2.0 * x * y
    xd = x * c + p1 * a + p2 * (r2 + 2.0 * x * x)
    yd = y * c + p1 * (r2 + 2.0 * y * y) + p2 * a
    n = obj.shape[0]
    Ji = np.zeros((n, 2, NI))
    Ji[:, 0, 0], Ji[:, 1, 1], Ji[:, 0, 2], Ji[:, 1, 3] = xd, yd, 1.0, 1.0
    for col, pw in ((4, r2), (5, r4), (8, r6)):
        Ji[:, 0, col], Ji[:, 1, col] = fx * x * pw / den, fy * y * pw / den
    for col, pw in ((9, r2), (10, r4), (11, r6)):
        Ji[:, 0, col], Ji[:, 1, col] = -fx * x * c * pw / den, -fy * y * c * pw / den
    Ji[:, 0, 6], Ji[:, 1, 6] = fx * a, fy * (r2 + 2.0 * y * y)
    Ji[:, 0, 7], Ji[:, 1, 7] = fx * (r2 + 2.0 * x * x), fy * a
    Ji *= np.array([(mask >> i) & 1 for i in range(NI)], np.float64)
    cp = ((k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4) * den - num * (k4 + 2.0 * k5 * r2 + 3.0 * k6 * r4)) / (den * den)
    off = a * cp + 2.0 * p1 * x + 2.0 * p2 * y
    xx = c + 2.0 * x * x * cp + 2.0 * p1 * y + 6.0 * p2 * x
    yy = c + 2.0 * y * y * cp + 6.0 * p1 * y + 2.0 * p2 * x
    au = fx * np.stack([xx / z, off / z, -(xx * x + off * y) / z], -1)
    av = fy * np.stack([off / z, yy / z, -(off * x + yy * y) / z], -1)
    Jp = np.zeros((n, 2, 6))
    Jp[:, 0, :3], Jp[:, 0, 3:] = np.cross(q, au), au
    Jp[:, 1, :3], Jp[:, 1, 3:] = np.cross(q, av), av
    return Ji, Jp


def linearise(p, poses, obj, img, cmask, mask):
    """poses: {v: (R, t)} of the used views; cmask [V, n] the used corners -> the blocks of J^T J and J^T r"""
    lin = dict(A=np.zeros((NI, NI)), ga=np.zeros(NI), B={}, C={}, gb={}, cost=0.0, views=sorted(poses))
    for v in lin["views"]:
        R, t = poses[v]
        u = cmask[v]
        r = (project(p, R, t, obj[u]) - img[v][u]).reshape(-1)
        Ji, Jp = jacobians(p, R, t, obj[u], mask)
        Ji, Jp = Ji.reshape(-1, NI), Jp.reshape(-1, 6)
        lin["A"] += Ji.T @ Ji
        lin["ga"] += Ji.T @ r
        lin["B"][v], lin["C"][v], lin["gb"][v] = Jp.T @ Jp, Ji.T @ Jp, Jp.T @ r
        lin["cost"] += float(r @ r)
    return lin


def cost_of(p, poses, obj, img, cmask):
    c = 0.0
    for v in sorted(poses):
        u = cmask[v]
        r = project(p, poses[v][0], poses[v][1], obj[u]) - img[v][u]
        c += float((r * r).sum())
    return c


# ---- rule 6 -------------------------------------------------------------------------------------------------------------
def reduced_system(lin, lam, mask):
    """S and its right side, fixed intrinsics as identity rows; also every view's B*^-1"""
    fixed = np.array([not (mask >> i) & 1 for i in range(NI)])
    S = lin["A"] + lam * np.diag(np.diag(lin["A"]))
    rhs = -lin["ga"].copy()
    Binv = {}
    for v in lin["views"]:
        Bs = lin["B"][v] + lam * np.diag(np.diag(lin["B"][v]))
        Binv[v] = np.linalg.inv(Bs)
        S -= lin["C"][v] @ Binv[v] @ lin["C"][v].T
        rhs += lin["C"][v] @ Binv[v] @ lin["gb"][v]
    S[fixed, :] = 0.0
    S[:, fixed] = 0.0
    S[fixed, fixed] = 1.0
    rhs[fixed] = 0.0
    return S, rhs, Binv


def schur_step(lin, lam, mask):
    S, rhs, Binv = reduced_system(lin, lam, mask)
    da = np.linalg.solve(S, rhs)
    return da, {v: -Binv[v] @ (lin["gb"][v] + lin["C"][v].T @ da) for v in lin["views"]}


def dense_system(lin, mask):
    """H = J^T J and g = J^T r over (free intrinsics, then 6 per view), for the tests"""
    fr = [i for i in range(NI) if (mask >> i) & 1]
    nv, nf = len(lin["views"]), len(fr)
    H, g = np.zeros((nf + 6 * nv, nf + 6 * nv)), np.zeros(nf + 6 * nv)
    H[:nf, :nf], g[:nf] = lin["A"][np.ix_(fr, fr)], lin["ga"][fr]
    for k, v in enumerate(lin["views"]):
        sl = slice(nf + 6 * k, nf + 6 * k + 6)
        H[sl, sl], H[:nf, sl], H[sl, :nf], g[sl] = lin["B"][v], lin["C"][v][fr], lin["C"][v][fr].T, lin["gb"][v]
    return H, g


# ---- rules 2 and 3 --------------------------------------------------------------------------------------------------------
def start_intrinsics(Hn, views, width, height):
    cx, cy = (width - 1.0) / 2.0, (height - 1.0) / 2.0
    rows = []
    for v in views:
        Hc = np.array([[1.0, 0.0, -cx], [0.0, 1.0, -cy], [0.0, 0.0, 1.0]]) @ Hn[v]
        h, w = Hc[:, 0], Hc[:, 1]
        d1, d2 = (h + w) / 2.0, (h - w) / 2.0
        h, w, d1, d2 = (x / np.linalg.norm(x) for x in (h, w, d1, d2))
        rows += [[h[0] * w[0], h[1] * w[1], -h[2] * w[2]], [d1[0] * d2[0], d1[1] * d2[1], -d1[2] * d2[2]]]
    rows = np.array(rows)
    N, r = rows[:, :2].T @ rows[:, :2], rows[:, :2].T @ rows[:, 2]
    det = N[0, 0] * N[1, 1] - N[0, 1] * N[0, 1]
    with np.errstate(all="ignore"):
        fa, fb = (N[1, 1] * r[0] - N[0, 1] * r[1]) / det, (N[0, 0] * r[1] - N[0, 1] * r[0]) / det
        return np.array([np.sqrt(abs(1.0 / fa)), np.sqrt(abs(1.0 / fb)), cx, cy])


def start_pose(p, Hn):
    Kinv = np.array([[1.0 / p[0], 0.0, -p[2] / p[0]], [0.0, 1.0 / p[1], -p[3] / p[1]], [0.0, 0.0, 1.0]])
    M = Kinv @ Hn
    if M[2, 2] < 0:
        M = -M
    s = 1.0 / np.linalg.norm(M[:, 0])
    r1, r2 = s * M[:, 0], s * M[:, 1]
    U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], 1))
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return R, s * M[:, 2]


def log_so3(R):
    """cv2.Rodrigues(R) -> rvec, by the kernel's formulas"""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(a)
    c = min(max(0.5 * (np.trace(R) - 1.0), -1.0), 1.0)
    th = np.arctan2(sn, c)
    if c > -0.99:
        return (1.0 + th * th / 6.0 if sn < 1e-5 else th / sn) * a
    k = int(np.argmax(np.diag(R)))
    nk = np.sqrt(max((R[k, k] - c) / (1.0 - c), 0.0))
    nv = 0.5 * (R[k] + R[:, k]) / ((1.0 - c) * nk)
    nv[k] = nk
    return (-1.0 if nv @ a < 0 else 1.0) * th * nv


# ---- the solver -----------------------------------------------------------------------------------------------------------
def homographies(obj, img):
    V = img.shape[0]
    Hn, status = np.full((V, 3, 3), np.nan), np.zeros(V, bool)
    for v in range(V):
        f = bv.homography_fit(obj, img[v])
        Hn[v], status[v] = f["Hn"], f["status"]
    return Hn, status


def calibrate_group(obj, img, size, use, K0, dist0, mask, max_evals, Hn, status, start_scale=None, start_seed=0):
    """one group -> dict of its outputs.  start_scale, start_seed: the start's numbers are multiplied by 1 + start_scale
    uniform(-1, 1) (the tests' 1e-13 protocol)"""
    V, n = img.shape[:2]
    nan = np.nan
    cmask = np.isfinite(img).all(-1) & np.isfinite(obj).all(-1)[None]
    vused = (np.ones(V, bool) if use is None else np.asarray(use) != 0) & (cmask.sum(1) >= 4) & status
    views = [v for v in range(V) if vused[v]]
    nv, nc, nf = len(views), int(cmask[vused].sum()), bin(mask).count("1")
    out = dict(K=np.full((3, 3), nan), dist=np.full(12, nan), R=np.full((V, 3, 3), nan), t=np.full((V, 3), nan),
               rvec=np.full((V, 3), nan), err=np.full((V, n), nan), view_stats=np.full((V, 3), nan), rms=nan, cost0=nan, cost=nan,
               std=np.full(12, nan), n_evals=0, n_views=nv, n_corners=nc, success=0)
    if nv < 3 or 2 * nc < nf + 6 * nv:
        return out
    p = np.zeros(NI)
    if dist0 is not None:
        p[4:] = np.asarray(dist0, np.float64)[:8]
    if K0 is not None:
        p[:4] = K0[0, 0], K0[1, 1], K0[0, 2], K0[1, 2]
    else:
        p[:4] = start_intrinsics(Hn, views, size[0], size[1])
    if not np.isfinite(p).all() or p[0] == 0 or p[1] == 0:
        return out
    poses = {v: start_pose(p, Hn[v]) for v in views}
    if start_scale is not None:
        rng = np.random.default_rng(start_seed)
        p = p * (1 + start_scale * rng.uniform(-1, 1, NI))
        poses = {v: (R * (1 + start_scale * rng.uniform(-1, 1, (3, 3))), t * (1 + start_scale * rng.uniform(-1, 1, 3)))
                 for v, (R, t) in poses.items()}
    free = np.array([(mask >> i) & 1 for i in range(NI)], bool)
    with np.errstate(all="ignore"):
        lin = linearise(p, poses, obj, img, cmask, mask)
        c = c0 = lin["cost"]
        if not np.isfinite(c):
            return out
        evals, lam, success = 1, LAM0, 0
        while evals < max_evals:
            da, dv = schur_step(lin, lam, mask)
            pt = np.where(free, p + da, p)
            trial = {v: (rr.exp_so3(dv[v][:3]) @ poses[v][0], poses[v][1] + dv[v][3:]) for v in views}
            ct = cost_of(pt, trial, obj, img, cmask)
            evals += 1
            if np.isfinite(ct) and ct <= c * (1.0 + 1e-14):
                dn2 = float((da[free] ** 2).sum() + sum((dv[v] ** 2).sum() for v in views))
                xn2 = float((pt[free] ** 2).sum() + sum((trial[v][1] ** 2).sum() for v in views))
                p, poses = pt, trial
                lam = max(lam / 10.0, LAM_MIN)
                lin = linearise(p, poses, obj, img, cmask, mask)
                c = lin["cost"]
                if np.sqrt(dn2) <= TAU * (1.0 + np.sqrt(xn2)):
                    success = 1
                    break
            else:
                lam = 10.0 * lam
                if not lam < LAM_MAX:
                    break
        # rule 9
        m, npar = 2 * nc, nf + 6 * nv
        S0, _, _ = reduced_system(lin, 0.0, mask)
        std = np.full(12, nan)
        ok = m > npar and all((np.linalg.eigvalsh(lin["B"][v]) > 0).all() for v in views)
        if ok:
            try:
                np.linalg.cholesky(S0)
                std = np.where(free, np.sqrt(np.diag(np.linalg.inv(S0)) * c / (m - npar)), nan)
            except np.linalg.LinAlgError:
                pass
        out.update(K=np.array([[p[0], 0.0, p[2]], [0.0, p[1], p[3]], [0.0, 0.0, 1.0]]), dist=dist12(p), rms=np.sqrt(c / nc), cost0=c0,
                   cost=c, std=std, n_evals=evals, success=success)
        for v in views:
            R, t = poses[v]
            d = project(p, R, t, obj) - img[v]
            e = np.where(cmask[v], np.sqrt((d * d).sum(-1)), nan)
            k = cmask[v].sum()
            out["R"][v], out["t"][v], out["rvec"][v], out["err"][v] = R, t, log_so3(R), e
            out["view_stats"][v] = np.nansum(e) / k, np.sqrt(np.nansum(e * e) / k), np.nanmax(e)
    return out


def calibrate_camera(obj, img, image_size, use=None, K0=None, dist0=None, mask=None, max_evals=200, start_scale=None, start_seed=0):
    """obj [n, 2], img [V, n, 2], use [G, V] | None, K0 [G, 3, 3] | None, dist0 [G, 12] | None -> dict of arrays with a
    leading group axis"""
    obj, img = np.asarray(obj, np.float64), np.asarray(img, np.float64)
    mask = free_mask() if mask is None else mask
    G = 1 if use is None else len(use)
    if use is None and K0 is not None:
        G = len(K0)
    Hn, status = homographies(obj, img)
    groups = [calibrate_group(obj, img, image_size, None if use is None else use[g], None if K0 is None else K0[g],
                              None if dist0 is None else dist0[g], mask, max_evals, Hn, status, start_scale, start_seed) for g in range(G)]
    return {k: np.stack([np.asarray(x[k]) for x in groups]) for k in groups[0]}
