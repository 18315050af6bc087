"""Float64 NumPy restatement of csrc/evaluate.hip, written from the rules of include/skimi.h (DESIGN §2 "Evaluation"):
pose_errors (the MPJPE protocols, the per-joint tables) and clip_quality (the ground-truth-free figures), vectorised over a
clip's frames.  tests/test_evaluate_cpu.py holds it against the reference's own functions (tests/golden/evaluate.npz);
tests/test_evaluate_gpu.py holds the device against it."""
import warnings

import numpy as np

NAN = float("nan")
H36M_EDGES = ((0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13), (8, 14),
              (14, 15), (15, 16))
H36M_LR_PAIRS = ((4, 1), (5, 2), (6, 3), (14, 11), (15, 12), (16, 13))
H36M_LEFT_BONES = ((0, 4), (4, 5), (5, 6), (8, 14), (14, 15), (15, 16))
H36M_RIGHT_BONES = ((0, 1), (1, 2), (2, 3), (8, 11), (11, 12), (12, 13))
PE_FRAME_FLOATS = ("err", "p_err", "vel_err", "mpjpe_f", "n_mpjpe_f", "p_mpjpe_f", "aligned", "p_R", "p_scale", "p_t")
PE_CLIP_FLOATS = ("mpjpe", "p_mpjpe", "n_mpjpe", "mpjve", "joint_err", "joint_p_err")
PE_EXACT = ("n_valid_f", "p_status", "n_err", "n_complete", "n_vel", "joint_err_n", "joint_p_err_n")
CQ_SCALARS = ("bone_cv_pooled", "bone_cv_mean", "lr_length_symmetry", "speed_mean", "jerk_mean", "speed_p95", "accel_p95",
              "mirror_symmetry")
CQ_FLOATS = CQ_SCALARS + ("bone_cv_edge", "bone_len")


def _norm(d):
    return np.sqrt((d * d).sum(axis=-1))


def _finite_mean(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    a = a[np.isfinite(a)]
    return (float(a.mean()) if a.size else NAN), int(a.size)


def _lengths(lengths, B, T):
    return np.full(B, T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths, dtype=np.int64), 0, T)


def procrustes(p, g):
    """rule 4 on complete frames p, g [n, J, 3] -> p_err [n, J], aligned, R, scale, t, status [n]"""
    n, J = p.shape[:2]
    muX, muY = g.mean(axis=1, keepdims=True), p.mean(axis=1, keepdims=True)
    X0, Y0 = g - muX, p - muY
    nX, nY = np.sqrt((X0 ** 2).sum(axis=(1, 2))), np.sqrt((Y0 ** 2).sum(axis=(1, 2)))
    ok = (nX > 0) & (nY > 0) & np.isfinite(nX) & np.isfinite(nY)
    sX, sY = np.where(ok, nX, 1.0), np.where(ok, nY, 1.0)
    H = np.matmul((X0 / sX[:, None, None]).transpose(0, 2, 1), Y0 / sY[:, None, None])
    ok &= np.isfinite(H).all(axis=(1, 2))
    H = np.where(ok[:, None, None], H, np.eye(3))
    U, s, Vt = np.linalg.svd(H)
    V = Vt.transpose(0, 2, 1).copy()
    sign = np.sign(np.linalg.det(np.matmul(V, U.transpose(0, 2, 1))))
    V[:, :, -1] *= sign[:, None]
    s = s.copy()
    s[:, -1] *= sign
    R = np.matmul(V, U.transpose(0, 2, 1))
    a = s.sum(axis=1) * sX / sY
    t = muX - a[:, None, None] * np.matmul(muY, R)
    aligned = a[:, None, None] * np.matmul(p, R) + t
    p_err = _norm(aligned - g)
    ok &= np.isfinite(p_err.mean(axis=1)) & np.isfinite(a) & np.isfinite(t).all(axis=(1, 2)) & np.isfinite(R).all(axis=(1, 2))
    bad = ~ok
    p_err[bad], aligned[bad], R[bad], a[bad], t[bad] = NAN, NAN, NAN, NAN, NAN
    return p_err, aligned, R, a, t[:, 0], ok


def singular_values(p, g):
    """the singular values of rule 4's H on complete frames with extent -> [n, 3], descending"""
    X0, Y0 = g - g.mean(axis=1, keepdims=True), p - p.mean(axis=1, keepdims=True)
    nX, nY = np.sqrt((X0 ** 2).sum(axis=(1, 2))), np.sqrt((Y0 ** 2).sum(axis=(1, 2)))
    ok = (nX > 0) & (nY > 0)
    H = np.matmul((X0[ok] / nX[ok, None, None]).transpose(0, 2, 1), Y0[ok] / nY[ok, None, None])
    return np.linalg.svd(H, compute_uv=False)


def joint_table(e):
    """e [n, J] -> (mean, std, median) [J, 3], n [J] over each joint's finite samples"""
    J = e.shape[1]
    out, cnt = np.full((J, 3), NAN), np.zeros(J, dtype=np.int32)
    for j in range(J):
        a = e[:, j][np.isfinite(e[:, j])]
        cnt[j] = a.size
        if a.size:
            out[j] = a.mean(), a.std(), np.median(a)
    return out, cnt


def pose_errors_clip(p, g, zero_root=-1):
    """one clip p, g [n, J, 3] -> dict of the per-frame and per-clip outputs"""
    n, J = p.shape[:2]
    g = g.copy()
    if zero_root is not None and zero_root >= 0:
        g[:, zero_root] = 0.0
    r = {}
    with np.errstate(all="ignore"):
        valid = np.isfinite(p).all(axis=2) & np.isfinite(g).all(axis=2)
        err = np.where(valid, _norm(p - g), NAN)
        fin = np.isfinite(err)
        cnt = fin.sum(axis=1)
        r["err"] = err
        r["mpjpe_f"] = np.where(cnt > 0, np.where(fin, err, 0.0).sum(axis=1) / np.maximum(cnt, 1), NAN)
        r["n_valid_f"] = valid.sum(axis=1).astype(np.int32)
        complete = valid.all(axis=1) if J else np.zeros(n, dtype=bool)
        c = np.flatnonzero(complete)
        nf, pf = np.full(n, NAN), np.full(n, NAN)
        p_err, aligned = np.full((n, J), NAN), np.full((n, J, 3), NAN)
        R, a, t, status = np.full((n, 3, 3), NAN), np.full(n, NAN), np.full((n, 3), NAN), np.zeros(n, dtype=bool)
        if c.size:
            pc, gc = p[c], g[c]
            scale = (gc * pc).sum(axis=2).mean(axis=1) / (pc * pc).sum(axis=2).mean(axis=1)
            v = _norm(scale[:, None, None] * pc - gc).mean(axis=1)
            nf[c] = np.where(np.isfinite(v), v, NAN)
            p_err[c], aligned[c], R[c], a[c], t[c], status[c] = procrustes(pc, gc)
            pf[c] = p_err[c].mean(axis=1)
        r.update(n_mpjpe_f=nf, p_mpjpe_f=pf, p_err=p_err, aligned=aligned, p_R=R, p_scale=a, p_t=t, p_status=status)
        vel = np.full((n, J), NAN)
        if n >= 2:
            both = valid[1:] & valid[:-1]
            vel[1:] = np.where(both, _norm((p[1:] - p[:-1]) - (g[1:] - g[:-1])), NAN)
        r["vel_err"] = vel
    r["mpjpe"], r["n_err"] = _finite_mean(err)
    r["mpjve"], r["n_vel"] = _finite_mean(vel)
    r["p_mpjpe"], r["n_mpjpe"] = _finite_mean(pf)[0], _finite_mean(nf)[0]
    r["n_complete"] = int(complete.sum())
    r["joint_err"], r["joint_err_n"] = joint_table(err)
    r["joint_p_err"], r["joint_p_err_n"] = joint_table(p_err)
    return r


def pose_errors(pred, target, lengths=None, zero_root=None):
    """pred, target [B, T, J, 3] or [T, J, 3] -> dict of arrays with a leading clip axis, padded as the device pads"""
    P, G = np.asarray(pred, dtype=np.float64), np.asarray(target, dtype=np.float64)
    if P.ndim == 3:
        P, G = P[None], G[None]
    B, T, J = P.shape[:3]
    lens = _lengths(lengths, B, T)
    shapes = dict(err=(T, J), p_err=(T, J), vel_err=(T, J), mpjpe_f=(T,), n_mpjpe_f=(T,), p_mpjpe_f=(T,), aligned=(T, J, 3),
                  p_R=(T, 3, 3), p_scale=(T,), p_t=(T, 3))
    out = {k: np.full((B, *s), NAN) for k, s in shapes.items()}
    out.update(n_valid_f=np.zeros((B, T), dtype=np.int32), p_status=np.zeros((B, T), dtype=bool))
    for k in ("mpjpe", "p_mpjpe", "n_mpjpe", "mpjve"):
        out[k] = np.full(B, NAN)
    for k in ("n_err", "n_complete", "n_vel"):
        out[k] = np.zeros(B, dtype=np.int32)
    out.update(joint_err=np.full((B, J, 3), NAN), joint_p_err=np.full((B, J, 3), NAN), joint_err_n=np.zeros((B, J), dtype=np.int32),
               joint_p_err_n=np.zeros((B, J), dtype=np.int32))
    for b in range(B):
        n = int(lens[b])
        r = pose_errors_clip(P[b, :n], G[b, :n], -1 if zero_root is None else zero_root)
        for k, v in r.items():
            if k in shapes or k in ("n_valid_f", "p_status"):
                out[k][b, :n] = v
            else:
                out[k][b] = v
    return out


def bone_lengths(X, edges):
    """X [n, J, 3] -> L [n, E], NaN unless both endpoints are finite"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    A, Bp = X[:, e[:, 0]], X[:, e[:, 1]]
    with np.errstate(all="ignore"):
        L = _norm(Bp - A)
    L[~(np.isfinite(A).all(axis=2) & np.isfinite(Bp).all(axis=2))] = NAN
    return L


def _nanmean(L):
    L = L[~np.isnan(L)]
    return float(L.mean()) if L.size else NAN


def fill_series(X):
    """np.interp over the frame index of every (joint, coordinate) series with at least 2 finite samples"""
    Xf = X.copy()
    n, J = X.shape[:2]
    t = np.arange(n)
    for j in range(J):
        for c in range(3):
            m = np.isfinite(X[:, j, c])
            if m.sum() >= 2:
                Xf[:, j, c] = np.interp(t, t[m], X[m, j, c])
    return Xf


def clip_quality_clip(X, edges, left_edges, right_edges, lr_pairs):
    n, J = X.shape[:2]
    r = {}
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        L = bone_lengths(X, edges)
        r["bone_len"] = L
        ok = ~np.isnan(L)
        r["bone_cv_pooled"] = float(L[ok].std() / (L[ok].mean() + 1e-9)) if ok.any() else NAN
        cv = np.full(L.shape[1], NAN)
        for e in range(L.shape[1]):
            a = L[ok[:, e], e]
            if a.size and a.mean() > 1e-9:
                cv[e] = a.std() / a.mean()
        r["bone_cv_edge"] = cv
        has = [e for e in range(L.shape[1]) if ok[:, e].any() and L[ok[:, e], e].mean() > 1e-9]
        r["bone_cv_mean"] = float(np.mean(cv[has])) if has else NAN
        Lm, Rm = _nanmean(bone_lengths(X, left_edges)), _nanmean(bone_lengths(X, right_edges))
        r["lr_length_symmetry"] = abs(Lm - Rm) / (0.5 * (Lm + Rm) + 1e-9)
        for k in ("speed_mean", "jerk_mean", "speed_p95", "accel_p95"):
            r[k] = NAN
        if n >= 3:
            v = X[1:] - X[:-1]
            okv = np.isfinite(v).all(axis=2)
            r["speed_mean"] = float(_norm(v[okv]).mean()) if okv.any() else NAN
            a = v[1:] - v[:-1]
            oka = np.isfinite(a).all(axis=2)
            r["jerk_mean"] = float(_norm(a[oka]).mean()) if oka.any() else NAN
            Xf = fill_series(X)
            r["speed_p95"] = float(np.percentile(_norm(np.diff(Xf, axis=0)), 95))
            r["accel_p95"] = float(np.percentile(_norm(np.diff(Xf, n=2, axis=0)), 95))
        d = []
        if n >= 1:
            last = X[n - 1]
            for l, rr in lr_pairs:
                if np.isfinite(last[l]).all() and np.isfinite(last[rr]).all():
                    d.append(_norm(last[l] - last[rr] * np.array([-1.0, 1.0, 1.0])))
        r["mirror_symmetry"] = float(np.mean(d)) if d else NAN
    return r


def clip_quality(X, lengths=None, edges=H36M_EDGES, left_edges=H36M_LEFT_BONES, right_edges=H36M_RIGHT_BONES, lr_pairs=H36M_LR_PAIRS):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 3:
        X = X[None]
    B, T, J = X.shape[:3]
    lens = _lengths(lengths, B, T)
    E = len(edges)
    out = {k: np.full(B, NAN) for k in CQ_SCALARS}
    out.update(bone_cv_edge=np.full((B, E), NAN), bone_len=np.full((B, T, E), NAN))
    for b in range(B):
        n = int(lens[b])
        r = clip_quality_clip(X[b, :n], edges, left_edges, right_edges, lr_pairs)
        out["bone_len"][b, :n] = r.pop("bone_len")
        for k, v in r.items():
            out[k][b] = v
    return out


def evaluate_clips(preds, targets, zero_root=0):
    """run.py:998-1041's aggregation on top of pose_errors_clip: sum T_i metric_i / sum T_i x 1000"""
    tot, N = np.zeros(4), 0
    for p, g in zip(preds, targets):
        r = pose_errors_clip(np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64), -1 if zero_root is None else zero_root)
        T = p.shape[0]
        tot += T * np.array([r["mpjpe"], r["p_mpjpe"], r["n_mpjpe"], r["mpjve"]])
        N += T
    return tuple(tot / N * 1000.0)


FUSED_METRIC_KEYS = ("L-R MeanDist (Before)", "Fused-Left MeanDist", "Fused-Right MeanDist", "L/R→Fused Gain (approx)",
                     "Bone Length CV", "LR Length Symmetry", "Speed P95", "Accel P95", "Symmetry Score (mirror)")


def eval_fused_pose(left, right, fused):
    k = FUSED_METRIC_KEYS
    m = {k[0]: pose_errors_clip(left, right)["mpjpe"], k[1]: pose_errors_clip(fused, left)["mpjpe"],
         k[2]: pose_errors_clip(fused, right)["mpjpe"]}
    m[k[3]] = m[k[0]] - 0.5 * (m[k[1]] + m[k[2]])
    q = clip_quality_clip(fused, H36M_EDGES, H36M_LEFT_BONES, H36M_RIGHT_BONES, H36M_LR_PAIRS)
    m[k[4]], m[k[5]] = q["bone_cv_pooled"], q["lr_length_symmetry"]
    if fused.shape[0] >= 3:
        m[k[6]], m[k[7]] = q["speed_p95"], q["accel_p95"]
    m[k[8]] = q["mirror_symmetry"]
    return m


def worst(got, want):
    """max |got - want| / (1 + |want|) over the finite entries of want; the NaN masks must agree (inf where they do not)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    m = ~np.isnan(want)
    if not m.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(got[m] - want[m]) / (1.0 + np.abs(want[m]))
    d = np.where((got[m] == want[m]), 0.0, d)             # equal infinities
    return float(d.max())
