"""Float64 NumPy restatement of the outlier-robust triangulation (DESIGN §2 "Robust triangulation"; the rules in
include/skimi.h above skimi_triangulate_robust), written from the rules, one function per rule, to be read top to bottom.
It imports nothing from the package.  The DLT is numpy.linalg.eigh of the 4 x 4 system (the kernel: cyclic Jacobi), the
Gauss-Newton solve numpy.linalg.solve (the kernel: LDL^T).

Besides the results every function returns what the tests need to check their margins: the errors of every scoring,
every hypothesis' key and inlier set, the eigenvalues of every system that was solved."""
import itertools

import numpy as np

NAN3 = np.full(3, np.nan)


def cameras(K, R, t):
    """P_v = K_v [R_v | t_v]: K, R [V, 3, 3], t [V, 3] -> [V, 3, 4]"""
    K, R, t = (np.asarray(a, np.float64) for a in (K, R, t))
    return np.stack([K[v] @ np.concatenate([R[v], t[v][:, None]], axis=1) for v in range(len(K))])


def eligible(kp, conf, conf_thr):
    """rule 1: kp [V, 2], conf [V] | None -> bool [V]: both coordinates finite and (no scores or score >= conf_thr)"""
    el = np.isfinite(kp).all(axis=1)
    if conf is not None:
        with np.errstate(invalid="ignore"):
            el &= np.asarray(conf, np.float64) >= conf_thr          # a NaN score compares false
    return el


def weights(conf, weighted, V):
    """rule 8: w_v = 1 without weighting or scores; else the score clipped to [0, 1], a non-finite one -> 0"""
    if not weighted or conf is None:
        return np.ones(V)
    c = np.asarray(conf, np.float64)
    return np.where(np.isfinite(c), np.minimum(np.maximum(c, 0.0), 1.0), 0.0)


def set_weights(w, views):
    """rule 8, last sentence: a set whose weights leave fewer than two views with w_v > 0 is taken unweighted"""
    return w if sum(w[v] > 0 for v in views) >= 2 else np.ones_like(w)


def dlt(P, kp, views, w=None):
    """The DLT over `views` (rows of view v times w_v): the eigenvector of A^T A for its smallest eigenvalue, divided by
    its last component -> (X [3], eigenvalues [4] ascending | None).  A non-finite system has no solution: (NaN, None)."""
    rows = []
    for v in views:
        s = 1.0 if w is None else w[v]
        rows.append(s * (kp[v, 0] * P[v, 2] - P[v, 0]))
        rows.append(s * (kp[v, 1] * P[v, 2] - P[v, 1]))
    A = np.array(rows)
    M = A.T @ A
    if not np.isfinite(M).all():
        return NAN3.copy(), None
    lam, Q = np.linalg.eigh(M)
    q = Q[:, 0]
    with np.errstate(all="ignore"):
        return q[:3] / q[3], lam


def project(P, X):
    """-> (pixels [V, 2], depth z [V]) of X through every P_v, plain division"""
    p = P @ np.append(X, 1.0)
    with np.errstate(all="ignore"):
        return p[:, :2] / p[:, 2:3], p[:, 2]


def errors(P, kp, X):
    """e_v = ||pi_v(X) - keypoint_v|| for every view (NaN where anything is NaN) and the depths"""
    uv, z = project(P, X)
    with np.errstate(all="ignore"):
        return np.sqrt(((uv - kp) ** 2).sum(axis=1)), z


def score(P, kp, elig, X, thr):
    """rule 3 -> dict(e [V] (NaN for a view that is not eligible), inliers (tuple of views), cost)"""
    e, z = errors(P, kp, X)
    inl, cost = [], 0.0
    for v in range(len(P)):                       # view order
        if not elig[v]:
            continue
        if z[v] > 0 and e[v] <= thr:
            inl.append(v)
        c = min(e[v], thr) if (z[v] > 0 and np.isfinite(e[v])) else thr
        cost += c * c
    return dict(e=np.where(elig, e, np.nan), inliers=tuple(inl), cost=cost)


def hypotheses(P, kp, elig, thr):
    """rule 2: every pair a < b of eligible views in lexicographic order -> list of dict(pair, X, skipped, eig, + score)"""
    out = []
    for a, b in itertools.combinations([v for v in range(len(P)) if elig[v]], 2):
        X, lam = dlt(P, kp, (a, b))
        if lam is None or not np.isfinite(X).all():
            out.append(dict(pair=(a, b), X=X, skipped=True, eig=lam))
            continue
        out.append(dict(pair=(a, b), X=X, skipped=False, eig=lam, **score(P, kp, elig, X, thr)))
    return out


def select(hyps):
    """rule 4: most inliers, then the smaller cost, then the earlier pair -> index into hyps | None (fails)"""
    best = None
    for i, h in enumerate(hyps):
        if h["skipped"]:
            continue
        if best is None or (len(h["inliers"]), -h["cost"]) > (len(hyps[best]["inliers"]), -hyps[best]["cost"]):
            best = i
    if best is None or len(hyps[best]["inliers"]) < 2:
        return None
    return best


def refit(P, kp, elig, w, thr, X, inl):
    """rule 5 from the winning hypothesis (X, inl) -> (X, inliers, rounds); rounds: one dict per round with the set that
    was fitted, the fit, its scoring and what happened (fallback / changed)"""
    rounds = []
    for _ in range(3):
        Xn, lam = dlt(P, kp, inl, set_weights(w, inl))
        sc = score(P, kp, elig, Xn, thr)
        rounds.append(dict(fitted=inl, X=Xn, eig=lam, fallback=len(sc["inliers"]) < 2, changed=sc["inliers"] != inl, **sc))
        if len(sc["inliers"]) < 2:
            break                                  # the previous X and set stay
        X, same, inl = Xn, sc["inliers"] == inl, sc["inliers"]
        if same:
            break
    return X, inl, rounds


def reprojection_cost(P, kp, w, inl, X):
    """c(X) = sum over the set, in view order, of w_v^2 ||pi_v(X) - keypoint_v||^2"""
    uv, _ = project(P, X)
    c = 0.0
    with np.errstate(all="ignore"):
        for v in inl:
            c += w[v] * w[v] * ((uv[v, 0] - kp[v, 0]) ** 2 + (uv[v, 1] - kp[v, 1]) ** 2)
    return c


def residuals(P, kp, w, inl, X):
    """the stacked weighted residuals w_v (pi_v(X) - keypoint_v) whose squared norm is c(X) (for scipy's least_squares)"""
    uv, _ = project(P, X)
    return np.concatenate([w[v] * (uv[v] - kp[v]) for v in inl])


def cost_change(P, kp, w, inl, X, d):
    """c(X + d) - c(X), formed from the step and not from two rounded sums: with u = pi_v(X), r = u - keypoint_v and
    (a, b) = P_v[:, :3] d, the residual moves by dr = (a_xy - u b) / (z + b), and |r + dr|^2 - |r|^2 = dr . (2 r + dr).
    Summed in view order.  Comparing c(X + d) with c(X) as two float64 numbers cannot see a decrease under eps c, i.e. a
    step under ~1e-10, and which side of that a step falls on depends on the last bits of X; this difference keeps its
    sign down to steps of a few ulp of X."""
    dc = 0.0
    with np.errstate(all="ignore"):
        for v in inl:
            p = P[v] @ np.append(X, 1.0)
            u = p[:2] / p[2]
            r = u - kp[v]
            ab = P[v, :, :3] @ d
            dr = (ab[:2] - u * ab[2]) / (p[2] + ab[2])
            dc += w[v] * w[v] * (dr[0] * (2.0 * r[0] + dr[0]) + dr[1] * (2.0 * r[1] + dr[1]))
    return dc


def refine(P, kp, w, inl, X, iters):
    """rule 6 -> (X, steps taken, True if a step was computed and rejected).  The step that is judged is the one X can
    take in float64, (X + d) - X."""
    w = set_weights(w, inl)
    taken = 0
    for _ in range(iters):
        H, g = np.zeros((3, 3)), np.zeros(3)
        for v in inl:
            p = P[v] @ np.append(X, 1.0)
            r = p[:2] / p[2] - kp[v]
            Jm = (P[v, :2, :3] * p[2] - np.outer(p[:2], P[v, 2, :3])) / p[2] ** 2      # d pi_v / d X, 2 x 3
            H += w[v] * w[v] * (Jm.T @ Jm)
            g += w[v] * w[v] * (Jm.T @ r)
        try:
            d = np.linalg.solve(H, -g)
        except np.linalg.LinAlgError:
            return X, taken, True
        Xn = X + d
        if not np.isfinite(Xn).all():
            return X, taken, True
        if not cost_change(P, kp, w, inl, X, Xn - X) < 0:
            return X, taken, True
        X, taken = Xn, taken + 1
    return X, taken, False


def joint(P, kp, conf=None, conf_thr=0.3, inlier_px=2.0, min_inliers=2, refine_iters=5, weighted=False):
    """rules 1 - 7 for one joint: P [V, 3, 4], kp [V, 2], conf [V] | None -> dict(X, err, inliers, mask, rms, ok, failed
    and the trace: elig, hyps, winner, rounds, gn_taken, gn_rejected)"""
    V = len(P)
    finite_kp = np.isfinite(kp).all(axis=1)
    elig = eligible(kp, conf, conf_thr)
    w = weights(conf, weighted, V)
    hyps = hypotheses(P, kp, elig, inlier_px)
    win = select(hyps)
    tr = dict(elig=elig, hyps=hyps, winner=win, rounds=[], gn_taken=0, gn_rejected=False)
    if win is None:                                # rule 7, a failed joint
        return dict(X=NAN3.copy(), err=np.full(V, np.nan), inliers=(), mask=0, rms=np.nan, ok=False, failed=True, **tr)
    X, inl, tr["rounds"] = refit(P, kp, elig, w, inlier_px, hyps[win]["X"], hyps[win]["inliers"])
    X, tr["gn_taken"], tr["gn_rejected"] = refine(P, kp, w, inl, X, refine_iters)
    e, _ = errors(P, kp, X)
    rms = float(np.sqrt(sum(e[v] * e[v] for v in inl) / len(inl)))
    ok = len(inl) >= min_inliers and bool(np.isfinite(X).all())
    return dict(X=X, err=np.where(finite_kp, e, np.nan), inliers=inl, mask=sum(1 << v for v in inl), rms=rms, ok=ok,
                failed=False, **tr)


def triangulate_robust(K, R, t, kp, conf=None, **kw):
    """K, R [T, V, 3, 3], t [T, V, 3], kp [T, V, J, 2], conf [T, V, J] | None -> the outputs of rule 7 as a dict of
    arrays (joints3d in float64: the caller rounds) + joints: the per-joint dicts [T][J]"""
    kp = np.asarray(kp, np.float64)
    T, V, J = kp.shape[:3]
    X, err = np.empty((T, J, 3)), np.empty((T, V, J))
    mask, rms = np.zeros((T, J), np.uint8), np.empty((T, J))
    ok, failed = np.zeros((T, J), bool), np.zeros((T, J), bool)
    ratio, report, joints = np.empty((T, V)), np.empty((T, 4)), []
    for i in range(T):
        P = cameras(K[i], R[i], t[i])
        row = []
        for j in range(J):
            r = joint(P, kp[i, :, j], None if conf is None else np.asarray(conf[i, :, j], np.float64), **kw)
            X[i, j], err[i, :, j], mask[i, j], rms[i, j], ok[i, j], failed[i, j] = r["X"], r["err"], r["mask"], r["rms"], r["ok"], r["failed"]
            row.append(r)
        joints.append(row)
        alive = [r for r in row if not r["failed"]]
        ratio[i] = [sum(v in r["inliers"] for r in alive) / len(alive) for v in range(V)] if alive else np.nan
        good = [r for r in row if r["ok"]]
        sq = [r["rms"] ** 2 for r in good if not np.isnan(r["rms"])]                # joint order
        report[i] = [len(good), len(good) / J, sum(len(r["inliers"]) for r in good) / len(good) if good else np.nan,
                     np.sqrt(sum(sq) / len(sq)) if sq else np.nan]
    X_ok = X.copy()
    X_ok[~ok] = np.nan
    return dict(joints3d=X, err=err, inlier_views=mask, rms_px=rms, ok=ok, joints3d_ok=X_ok, view_inlier_ratio=ratio,
                report=report, failed=failed, joints=joints)


# ---- what the tests ask of an input before they compare discrete outputs ------------------------------------------------
def margins(res, inlier_px):
    """Over every joint of a triangulate_robust result -> dict(
    threshold: the smallest | e - inlier_px | over every error of every scoring (hypotheses and refit rounds),
    cost_tie: True if a hypothesis with the winner's inlier count and a cost within 1e-6 relative of the winner's has
              another inlier set,
    cond: the largest ratio lambda_max / lambda_2 over the systems that were solved (lambda_2: the second-smallest
          eigenvalue, the one that separates the solution from the rest))"""
    thr_m, tie, cond = np.inf, False, 0.0
    for row in res["joints"]:
        for r in row:
            scorings = [h for h in r["hyps"] if not h["skipped"]] + r["rounds"]
            for s in scorings:
                e = s["e"][np.isfinite(s["e"])]
                if e.size:
                    thr_m = min(thr_m, float(np.abs(e - inlier_px).min()))
                if s["eig"] is not None:
                    cond = max(cond, float(s["eig"][3] / s["eig"][1]))
            if r["winner"] is not None:
                wn = r["hyps"][r["winner"]]
                for h in r["hyps"]:
                    if h["skipped"] or len(h["inliers"]) != len(wn["inliers"]):
                        continue
                    if abs(h["cost"] - wn["cost"]) <= 1e-6 * abs(wn["cost"]) and h["inliers"] != wn["inliers"]:
                        tie = True
    return dict(threshold=thr_m, cost_tie=tie, cond=cond)
