"""Float64 NumPy restatement of the essential-matrix RANSAC (csrc/essential.hip; rules: DESIGN §2 "Essential matrix").
A problem is one group of correspondences; the groups are independent.  The statements follow the kernels', rule by rule.
What has to agree bit for bit does: the 9 x 9 A^T A of a sample (sums in point order) and its cyclic Jacobi (the same
rotations in the same order), because the four null vectors of a five-point sample span a degenerate eigenspace whose
basis is decided by rounding; everything after the basis is continuous in it and agrees to rounding.  The eigen-solve of
the action matrix is np.linalg.eig here (Hessenberg + Francis QR in the kernel); rule 4's polish is what makes them agree.

Reference: VideoPose3D/slove_rt_from_3d.py:114-121, :227-232; triangulation/camera_position/camera_position.py:88-117."""
import numpy as np

from resect_restated import jacobi, normalised_rays

MIN_POINTS = 5
MAX_SOLUTIONS = 10
JACOBI_SWEEPS = 60
PIVOT_TOL = 1e-14
POLISH_STEPS = 3           # measured: DESIGN §2 "Essential matrix"
RESIDUAL_BOUND = 1e-10     # on max |M mon| / (1 + x^2 + y^2 + z^2)^(3/2) after the polish; measured: DESIGN
MASK64 = (1 << 64) - 1

# monomials of degree <= 3 in (x, y, z) as sorted index triples over the variables (x, y, z, 1) = (0, 1, 2, 3)
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]
TRIPLES = [(i, j, k) for i in range(4) for j in range(i, 4) for k in range(j, 4)]
IDX2 = {p: n for n, p in enumerate(PAIRS)}
IDX3 = {t: n for n, t in enumerate(TRIPLES)}
# rule 4's order: x^3, x^2 y, x y^2, y^3, x^2 z, x y z, y^2 z, x z^2, y z^2, z^3 | x^2, x y, y^2, x z, y z, z^2, x, y, z, 1
ORDER = [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (0, 0, 2), (0, 1, 2), (1, 1, 2), (0, 2, 2), (1, 2, 2), (2, 2, 2),
         (0, 0, 3), (0, 1, 3), (1, 1, 3), (0, 2, 3), (1, 2, 3), (2, 2, 3), (0, 3, 3), (1, 3, 3), (2, 3, 3), (3, 3, 3)]
PERM = [IDX3[t] for t in ORDER]


# ---- rule 3 -----------------------------------------------------------------------------------------------------------
def splitmix64(s):
    s = (s + 0x9E3779B97F4A7C15) & MASK64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return s, z ^ (z >> 31)


def draw_sample(seed, g, h, m):
    """the five distinct ranks of hypothesis h of group g (g includes group_offset), m >= 5 used points"""
    s = (seed ^ (((g << 32) + h) & MASK64)) & MASK64
    s, _ = splitmix64(s)
    sample, outputs = [], 0
    while len(sample) < 5 and outputs < 64:
        s, z = splitmix64(s)
        outputs += 1
        r = z % m
        if r not in sample:
            sample.append(r)
    k = 0
    while len(sample) < 5:
        if k not in sample:
            sample.append(k)
        k += 1
    return sample


# ---- rule 4 -----------------------------------------------------------------------------------------------------------
def jacobi_batch(M):
    """resect_restated.jacobi on a stack [S, n, n], the same rotations in the same order per matrix -> (diag, Q)"""
    M = M.copy()
    S, n = M.shape[:2]
    Q = np.broadcast_to(np.eye(n), M.shape).copy()
    iu = np.triu_indices(n, 1)
    active = np.ones(S, bool)
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            off = np.zeros(S)
            diag = np.zeros(S)
            for a in range(n):                      # the kernel's order of these two sums
                diag = diag + M[:, a, a] * M[:, a, a]
                for b in range(a + 1, n):
                    off = off + M[:, a, b] * M[:, a, b]
            active = active & ~(~np.isfinite(off) | (off <= 1e-40 * diag) | (off == 0.0))
            if not active.any():
                break
            for p in range(n - 1):
                for q in range(p + 1, n):
                    mpq = M[:, p, q]
                    rot = active & (mpq != 0.0)
                    theta = (M[:, q, q] - M[:, p, p]) / (2.0 * mpq)
                    tn = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    cs = 1.0 / np.sqrt(tn * tn + 1.0)
                    sn = tn * cs
                    cs, sn = np.where(rot, cs, 1.0)[:, None], np.where(rot, sn, 0.0)[:, None]
                    keep = ~rot
                    mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = np.where(keep[:, None], mp, cs * mp - sn * mq)
                    M[:, :, q] = np.where(keep[:, None], mq, sn * mp + cs * mq)
                    mp, mq = M[:, p, :].copy(), M[:, q, :].copy()
                    M[:, p, :] = np.where(keep[:, None], mp, cs * mp - sn * mq)
                    M[:, q, :] = np.where(keep[:, None], mq, sn * mp + cs * mq)
                    M[:, p, q] = np.where(keep, M[:, p, q], 0.0)
                    M[:, q, p] = np.where(keep, M[:, q, p], 0.0)
                    qp, qq = Q[:, :, p].copy(), Q[:, :, q].copy()
                    Q[:, :, p] = np.where(keep[:, None], qp, cs * qp - sn * qq)
                    Q[:, :, q] = np.where(keep[:, None], qq, sn * qp + cs * qq)
    return np.stack([M[:, k, k] for k in range(n)], axis=1), Q


def nullspace_basis(a, b):
    """a, b [S, 5, 2] -> N [S, 4, 9]: the eigenvectors of the four smallest eigenvalues of A^T A, ascending, ties by index"""
    S = a.shape[0]
    ah = np.concatenate([a, np.ones((S, 5, 1))], axis=2)
    bh = np.concatenate([b, np.ones((S, 5, 1))], axis=2)
    rows = (bh[:, :, :, None] * ah[:, :, None, :]).reshape(S, 5, 9)
    AtA = np.zeros((S, 9, 9))
    for k in range(5):                              # sums in point order
        AtA = AtA + rows[:, k, :, None] * rows[:, k, None, :]
    d, Q = jacobi_batch(AtA)
    order = np.argsort(d, axis=1, kind="stable")[:, :4]
    return np.stack([np.take_along_axis(Q, order[:, None, k:k + 1], axis=2)[:, :, 0] for k in range(4)], axis=1)


def _mul11(p, q):
    out = np.zeros(p.shape[:-1] + (10,))
    for i in range(4):
        for j in range(4):
            out[..., IDX2[tuple(sorted((i, j)))]] += p[..., i] * q[..., j]
    return out


def _mul21(p, q):
    out = np.zeros(p.shape[:-1] + (20,))
    for n, (i, j) in enumerate(PAIRS):
        for k in range(4):
            out[..., IDX3[tuple(sorted((i, j, k)))]] += p[..., n] * q[..., k]
    return out


def constraint_matrix(N):
    """N [S, 4, 9] -> M [S, 10, 20]: det E = 0, then the entries of 2 E E^T E - tr(E E^T) E, over rule 4's monomials"""
    S = N.shape[0]
    e = [[N[:, :, 3 * r + c] for c in range(3)] for r in range(3)]        # linear polynomials [S, 4]
    rows = [_mul21(_mul11(e[1][1], e[2][2]) - _mul11(e[1][2], e[2][1]), e[0][0])
            - _mul21(_mul11(e[1][0], e[2][2]) - _mul11(e[1][2], e[2][0]), e[0][1])
            + _mul21(_mul11(e[1][0], e[2][1]) - _mul11(e[1][1], e[2][0]), e[0][2])]
    eet = [[_mul11(e[i][0], e[j][0]) + _mul11(e[i][1], e[j][1]) + _mul11(e[i][2], e[j][2]) for j in range(3)] for i in range(3)]
    tr = eet[0][0] + eet[1][1] + eet[2][2]
    for i in range(3):
        for j in range(3):
            acc = np.zeros((S, 20))
            for k in range(3):
                lam = 2.0 * eet[i][k] - tr if i == k else 2.0 * eet[i][k]
                acc = acc + _mul21(lam, e[k][j])
            rows.append(acc)
    return np.stack(rows, axis=1)[:, :, PERM]


def eliminate(M):
    """M [S, 10, 20] -> (B [S, 10, 10] = M[:, :10]^-1 M[:, 10:], ok [S]) by Gauss-Jordan with partial pivoting"""
    A = M.copy()
    S = A.shape[0]
    ok = np.isfinite(A).all(axis=(1, 2))
    colmax = np.abs(M[:, :, :10]).max(axis=1)
    ar = np.arange(S)
    with np.errstate(all="ignore"):
        for c in range(10):
            piv = np.argmax(np.abs(A[:, c:, c]), axis=1) + c       # the first largest
            row_c, row_p = A[ar, c].copy(), A[ar, piv].copy()
            A[ar, piv] = row_c
            A[ar, c] = row_p
            p = A[:, c, c].copy()
            ok = ok & np.isfinite(p) & ~(np.abs(p) < PIVOT_TOL * colmax[:, c])
            A[:, c, :] = A[:, c, :] / p[:, None]
            for r in range(10):
                if r != c:
                    f = A[:, r, c].copy()
                    A[:, r, :] = A[:, r, :] - f[:, None] * A[:, c, :]
    return A[:, :, 10:], ok


def action_matrix(B):
    A = np.zeros(B.shape)
    for r, src in enumerate((0, 1, 2, 4, 5, 7)):
        A[:, r, :] = -B[:, src, :]
    A[:, 6, 0] = A[:, 7, 1] = A[:, 8, 3] = A[:, 9, 6] = 1.0
    return A


def monomials(x, y, z):
    """-> (mon [..., 20], d mon / d (x, y, z) [..., 20, 3]) in rule 4's order"""
    o, n = np.ones_like(x), np.zeros_like(x)
    mon = np.stack([x * x * x, x * x * y, x * y * y, y * y * y, x * x * z, x * y * z, y * y * z, x * z * z, y * z * z, z * z * z,
                    x * x, x * y, y * y, x * z, y * z, z * z, x, y, z, o], axis=-1)
    dx = np.stack([3 * x * x, 2 * x * y, y * y, n, 2 * x * z, y * z, n, z * z, n, n, 2 * x, y, n, z, n, n, o, n, n, n], axis=-1)
    dy = np.stack([n, x * x, 2 * x * y, 3 * y * y, n, x * z, 2 * y * z, n, z * z, n, n, x, 2 * y, n, z, n, n, o, n, n], axis=-1)
    dz = np.stack([n, n, n, n, x * x, x * y, y * y, 2 * x * z, 2 * y * z, 3 * z * z, n, n, n, x, y, 2 * z, n, n, o, n], axis=-1)
    return mon, np.stack([dx, dy, dz], axis=-1)


def constraint_residual(M, xyz):
    """M [S, 10, 20], xyz [S, C, 3] -> max |M mon| / (1 + |xyz|^2)^(3/2) [S, C]"""
    mon, _ = monomials(xyz[..., 0], xyz[..., 1], xyz[..., 2])
    r = np.einsum("sij,scj->sci", M, mon)
    return np.abs(r).max(axis=-1) / (1.0 + (xyz ** 2).sum(axis=-1)) ** 1.5


def polish(M, xyz, steps=POLISH_STEPS):
    """Gauss-Newton on the ten constraints: d = -(J^T J)^-1 J^T r by LDL^T without pivoting, `steps` times"""
    xyz = xyz.copy()
    with np.errstate(all="ignore"):
        for _ in range(steps):
            mon, dmon = monomials(xyz[..., 0], xyz[..., 1], xyz[..., 2])
            r = np.einsum("sij,scj->sci", M, mon)
            J = np.einsum("sij,scjk->scik", M, dmon)
            H = np.einsum("scik,scil->sckl", J, J)
            g = np.einsum("scik,sci->sck", J, r)
            d0 = H[..., 0, 0]
            l10, l20 = H[..., 1, 0] / d0, H[..., 2, 0] / d0
            d1 = H[..., 1, 1] - l10 * l10 * d0
            l21 = (H[..., 2, 1] - l20 * l10 * d0) / d1
            d2 = H[..., 2, 2] - l20 * l20 * d0 - l21 * l21 * d1
            y0 = -g[..., 0]
            y1 = -g[..., 1] - l10 * y0
            y2 = -g[..., 2] - l20 * y0 - l21 * y1
            s2 = y2 / d2
            s1 = y1 / d1 - l21 * s2
            s0 = y0 / d0 - l10 * s1 - l20 * s2
            xyz = xyz + np.stack([s0, s1, s2], axis=-1)
    return xyz


def roots_eig(A):
    """A [10, 10] -> candidates (x, y, z) [C, 3] from its real eigenpairs"""
    w, v = np.linalg.eig(A)
    out = [np.real(v[6:9, k] / v[9, k]) for k in range(10) if w[k].imag == 0.0 and v[9, k] != 0]
    return np.array(out).reshape(-1, 3)


def roots_charpoly(A):
    """the second route: real roots of the characteristic polynomial, then (A - lambda I)'s null vector by SVD"""
    out = []
    for lam in np.roots(np.poly(A)):
        if lam.imag != 0.0:
            continue
        v = np.linalg.svd(A - lam.real * np.eye(10))[2][-1]
        if v[9] != 0:
            out.append(v[6:9] / v[9])
    return np.array(out).reshape(-1, 3)


def five_point(a, b, roots=roots_eig, steps=POLISH_STEPS, details=False):
    """a, b [S, 5, 2] normalised coordinates -> (E [S, 10, 3, 3] NaN-padded, counts [S])"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    S = a.shape[0]
    N = nullspace_basis(a, b)
    M = constraint_matrix(N)
    B, ok = eliminate(M)
    A = action_matrix(B)
    cand = np.full((S, MAX_SOLUTIONS, 3), np.nan)
    for s in range(S):
        if ok[s] and np.isfinite(A[s]).all():
            c = roots(A[s])[:MAX_SOLUTIONS]
            cand[s, :len(c)] = c
    xyz = polish(M, cand, steps)
    with np.errstate(all="ignore"):
        res = constraint_residual(M, xyz)
    keep = np.isfinite(res) & (res < RESIDUAL_BOUND)
    E = np.full((S, MAX_SOLUTIONS, 3, 3), np.nan)
    counts = keep.sum(axis=1).astype(np.int32)
    sol = np.full((S, MAX_SOLUTIONS, 3), np.nan)
    for s in range(S):
        idx = np.nonzero(keep[s])[0]
        idx = idx[np.argsort(xyz[s, idx, 0], kind="stable")]
        for n, k in enumerate(idx):
            x, y, z = xyz[s, k]
            e = x * N[s, 0] + y * N[s, 1] + z * N[s, 2] + N[s, 3]
            E[s, n] = (e * (np.sqrt(2.0) / np.sqrt((e * e).sum()))).reshape(3, 3)
            sol[s, n] = xyz[s, k]
    if details:
        return E, counts, dict(N=N, M=M, A=A, ok=ok, xyz=sol, res=res, cand=cand)
    return E, counts


# ---- rules 1, 2 ---------------------------------------------------------------------------------------------------------
def mask(x2d, conf, min_conf):
    used = np.isfinite(x2d).all(axis=(0, 2))
    if conf is None:
        return used
    w = np.where(np.isfinite(conf), conf, 0.0)
    w = np.minimum(np.maximum(w, 0.0), 1.0)
    return used & (w >= min_conf).all(axis=0)


def tau_of(K, threshold):
    return threshold / ((K[0, 0, 0] + K[0, 1, 1] + K[1, 0, 0] + K[1, 1, 1]) / 4.0)


# ---- rule 5 -----------------------------------------------------------------------------------------------------------
def sampson(E, a, b):
    """E [..., 3, 3], a, b [m, 2] -> e^2 [..., m]"""
    ah = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1)
    bh = np.concatenate([b, np.ones((b.shape[0], 1))], axis=1)
    with np.errstate(all="ignore"):
        Ea = np.einsum("...ij,mj->...mi", E, ah)
        Etb = np.einsum("...ji,mj->...mi", E, bh)
        num = (Ea * bh).sum(axis=-1)
        return num * num / (Ea[..., 0] ** 2 + Ea[..., 1] ** 2 + Etb[..., 0] ** 2 + Etb[..., 1] ** 2)


def score(E, a, b, tau):
    e2 = sampson(E, a, b)
    inl = np.isfinite(e2) & (e2 <= tau * tau)
    cost = np.where(inl, e2, tau * tau).sum(axis=-1)
    return inl, cost, e2


# ---- rules 7, 8 ---------------------------------------------------------------------------------------------------------
def decompose(E):
    """-> the four candidates [(R, t)] in rule 7's order"""
    d, Q = jacobi(E.T @ E)
    k = int(np.argmin(d))
    v1, v2, v3 = Q[:, (k + 1) % 3], Q[:, (k + 2) % 3], Q[:, k]
    u1, u2 = E @ v1, E @ v2
    u1, u2 = u1 / np.sqrt((u1 * u1).sum()), u2 / np.sqrt((u2 * u2).sum())
    u3 = np.cross(u1, u2)
    U, V = np.stack([u1, u2, u3], axis=1), np.stack([v1, v2, v3], axis=1)
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Ra, Rb = U @ W @ V.T, U @ W.T @ V.T
    return [(Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3)]


def depths(R, t, a, b):
    """least-squares (z0, z1) of z0 (R a) - z1 b = -t per point"""
    ah = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1)
    bh = np.concatenate([b, np.ones((b.shape[0], 1))], axis=1)
    p = ah @ R.T
    pp, pb, bb = (p * p).sum(axis=1), (p * bh).sum(axis=1), (bh * bh).sum(axis=1)
    pt, bt = p @ t, bh @ t
    with np.errstate(all="ignore"):
        det = pp * bb - pb * pb
        return (pb * bt - pt * bb) / det, (pp * bt - pb * pt) / det


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


# ---- the whole ----------------------------------------------------------------------------------------------------------
def essential_ransac(x2d, K, conf=None, min_conf=0.0, group_size=None, threshold=1.0, hypotheses=1024, seed=0,
                     group_offset=0, baseline=1.0, distance_thresh=50.0, groups=None, details=False):
    """x2d [2, N, 2], K [2, 3, 3], conf [2, N] | None -> dict of rule 9's outputs (only `groups` are solved when given)"""
    x2d, K = np.asarray(x2d, np.float64), np.asarray(K, np.float64)
    N = x2d.shape[1]
    gs = N if group_size is None else int(group_size)
    G, H = N // gs, int(hypotheses)
    out = dict(R=np.full((G, 3, 3), np.nan), t=np.full((G, 3), np.nan), E=np.full((G, 3, 3), np.nan),
               inliers=np.zeros(N, np.uint8), pose_mask=np.zeros(N, np.uint8), n_used=np.zeros(G, np.int32),
               n_inliers=np.zeros(G, np.int32), n_pose=np.zeros(G, np.int32), cheirality=np.zeros((G, 4), np.int32),
               cost=np.full(G, np.nan), winner=np.full((G, 2), -1, np.int32), n_solutions=np.zeros(G, np.int32),
               confidence=np.full(G, np.nan), success=np.zeros(G, np.int32))
    used_all = mask(x2d, conf, min_conf)
    tau = tau_of(K, threshold)
    det = {}
    for g in (range(G) if groups is None else groups):
        sl = slice(g * gs, (g + 1) * gs)
        idx = np.nonzero(used_all[sl])[0]
        m = len(idx)
        out["n_used"][g] = m
        if m < MIN_POINTS:
            continue
        a = np.stack(normalised_rays(K[0], x2d[0, sl][idx]), axis=1)
        b = np.stack(normalised_rays(K[1], x2d[1, sl][idx]), axis=1)
        samples = np.array([draw_sample(seed, g + group_offset, h, m) for h in range(H)])
        E, counts = five_point(a[samples], b[samples])
        out["n_solutions"][g] = counts.sum()
        if counts.sum() == 0:
            continue
        inl, cost, e2 = score(E, a, b, tau)
        valid = np.arange(MAX_SOLUTIONS)[None] < counts[:, None]
        n_inl = np.where(valid, inl.sum(axis=-1), -1)
        hh, ss = np.nonzero(valid)
        order = np.lexsort((ss, hh, cost[hh, ss], -n_inl[hh, ss]))
        h, s = int(hh[order[0]]), int(ss[order[0]])
        Ew, win = E[h, s], inl[h, s]
        cands = decompose(Ew)
        ai, bi = a[win], b[win]
        passes, z4 = [], []
        for R, t in cands:
            z0, z1 = depths(R, t, ai, bi)
            z4.append(np.stack([z0, z1]))
            with np.errstate(invalid="ignore"):
                passes.append(np.isfinite(z0) & np.isfinite(z1) & (z0 > 0) & (z1 > 0) & (z0 < distance_thresh) & (z1 < distance_thresh))
        votes = np.array([p.sum() for p in passes])
        c = int(np.argmax(votes))
        R, t = cands[c]
        out["R"][g], out["t"][g], out["E"][g] = R, baseline * t, skew(t) @ R
        out["inliers"][sl][idx[win]] = 1
        out["pose_mask"][sl][idx[win][passes[c]]] = 1
        out["n_inliers"][g], out["n_pose"][g], out["cheirality"][g] = win.sum(), votes[c], votes
        out["cost"][g], out["winner"][g] = cost[h, s], (h, s)
        out["confidence"][g] = 1.0 - (1.0 - (win.sum() / m) ** 5) ** H
        out["success"][g] = int(win.sum() >= 5 and votes[c] > 0)
        if details:
            runner = order[1] if len(order) > 1 else None
            det[g] = dict(a=a, b=b, tau=tau, e2=e2[h, s], z=np.stack(z4), E_min=Ew,
                          runner=None if runner is None else (int(n_inl[hh[runner], ss[runner]]), float(cost[hh[runner], ss[runner]])))
    if details:
        out["details"] = det
    return out
