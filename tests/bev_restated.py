"""NumPy float64 restatement of the bird's-eye view (DESIGN §2 "Bird's-eye view"; rules: include/skimi.h), written from the
rules: the homography of four or more ground points (Hartley normalisation, the 9 x 9 normal matrix, cyclic Jacobi in
csrc/jacobi.h's sweep order, the eigenvector of the smallest eigenvalue: cv2.findHomography(method=0) without its
Levenberg-Marquardt polish), points through a homography, the perspective warp (cv2.warpPerspective(INTER_LINEAR), constant
border 0, positions and weights in float64), the skeleton on the plan, the ground track, the small pure functions of the
reference's bev_utils.py / front/run.py, and the chain of bev.process_front_clip.  Every expression is evaluated in the
order csrc/bev.hip evaluates it (no fused multiply-add on either side), the sums included: the fit adds over the points in
point order, as the kernel's lanes do, and the skeleton's centre is summed in the kernel's own wave order (wave_sum64), so that
half-way pixel values round alike.
"""
import numpy as np

from lens_restated import near_tie  # noqa: F401  (the same near-tie rule as the lens warp)

JACOBI_SWEEPS = 60
DEFAULT_IMG_PTS = np.array([[0.0, 1080.0], [1920.0, 1080.0], [1336.0, 130.0], [600.0, 130.0]])
DEFAULT_BEV_PTS_M = np.array([[-15.0, 0.0], [15.0, 0.0], [15.0, 60.0], [-15.0, 60.0]])


# ---- the reference's pure functions -------------------------------------------------------------------------------------
def make_bev_canvas(lane_width_m=30.0, lane_length_m=60.0, px_per_m=20.0, margin_x_m=5.0, margin_y_m=10.0):
    x_min, x_max = -lane_width_m / 2 - margin_x_m, lane_width_m / 2 + margin_x_m
    y_min, y_max = 0.0 - margin_y_m, lane_length_m + margin_y_m
    size = (int(np.ceil((x_max - x_min) * px_per_m)), int(np.ceil((y_max - y_min) * px_per_m)))
    s = px_per_m
    return size, np.array([[s, 0, -x_min * s], [0, -s, y_max * s], [0, 0, 1]], np.float64)


def foot_from_bbox_xyxy(b):
    b = np.asarray(b, np.float64)
    return np.stack([(b[..., 0] + b[..., 2]) * 0.5, b[..., 3]], -1)


def convert_xywh_to_xyxy(b):
    b = np.asarray(b)
    return np.stack([b[..., 0], b[..., 1], b[..., 0] + b[..., 2], b[..., 1] + b[..., 3]], -1)


def unnormalize_bbox(b, img_size):
    H, W = img_size
    return np.asarray(b, np.float64) * np.array([W, H, W, H], np.float64)


def apply3(M, x, y):
    """(X, Y, w) = M (x, y, 1), each component as (m0 x + m1 y) + m2"""
    M = np.asarray(M, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        return (M[0] * x + M[1] * y) + M[2], (M[3] * x + M[4] * y) + M[5], (M[6] * x + M[7] * y) + M[8]


def homography_points(x, H, eps=1e-8):
    """x [n, 2] through H [3, 3]: NaN in both coordinates where the point or w is non-finite or |w| < eps"""
    x = np.asarray(x, np.float64)
    X, Y, w = apply3(H, x[..., 0], x[..., 1])
    with np.errstate(all="ignore"):
        out = np.stack([X / w, Y / w], -1)
        bad = ~(np.isfinite(x[..., 0]) & np.isfinite(x[..., 1]) & np.isfinite(w)) | (np.abs(w) < eps)
    out[bad] = np.nan
    return out


# ---- the fit ------------------------------------------------------------------------------------------------------------
def jacobi(M):
    """csrc/jacobi.h: jacobi_serial -> (eigenvalues on the diagonal, eigenvectors in columns)"""
    M = np.array(M, np.float64)
    n = M.shape[0]
    Q = np.eye(n)
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            off = diag = 0.0
            for a in range(n):
                diag += M[a, a] * M[a, a]
                for b in range(a + 1, n):
                    off += M[a, b] * M[a, b]
            if not np.isfinite(off) or off <= 1e-40 * diag or off == 0.0:
                break
            for p in range(n - 1):
                for q in range(p + 1, n):
                    mpq = M[p, q]
                    if mpq == 0.0:
                        continue
                    theta = (M[q, q] - M[p, p]) / (2.0 * mpq)
                    tn = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    cs = 1.0 / np.sqrt(tn * tn + 1.0)
                    sn = tn * cs
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = cs * mp - sn * mq, sn * mp + cs * mq
                    mp, mq = M[p, :].copy(), M[q, :].copy()
                    M[p, :], M[q, :] = cs * mp - sn * mq, sn * mp + cs * mq
                    M[p, q] = M[q, p] = 0.0
                    qp, qq = Q[:, p].copy(), Q[:, q].copy()
                    Q[:, p], Q[:, q] = cs * qp - sn * qq, sn * qp + cs * qq
    return np.diag(M).copy(), Q


def det3(H):
    H = np.asarray(H, np.float64).reshape(9)
    return H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6])


def inverse3(H):
    """adj(H) / det(H), every cofactor a b - c d in written order"""
    h = np.asarray(H, np.float64).reshape(9)
    adj = np.array([h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                    h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                    h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]])
    with np.errstate(all="ignore"):
        return (adj / det3(h)).reshape(3, 3)


def compose3(A, B):
    """A @ B, every entry as (a0 b0 + a1 b1) + a2 b2"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def homography_fit(src, dst, post=None):
    """one group: src, dst [n, 2] -> dict(H, Hinv [3, 3], err [n], stats [4], status bool, Hn)"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = src.shape[0]
    post = np.eye(3) if post is None else np.asarray(post, np.float64)
    used = np.isfinite(src).all(1) & np.isfinite(dst).all(1)
    m = float(used.sum())
    nan9 = np.full((3, 3), np.nan)
    fail = dict(H=nan9, Hinv=nan9.copy(), err=np.full(n, np.nan), stats=np.array([m, np.nan, np.nan, np.nan]), status=False, Hn=nan9)
    if m < 4:
        return fail
    s, d = src[used], dst[used]
    with np.errstate(all="ignore"):
        def seq(v):
            t = 0.0
            for e in v:
                t += e
            return t
        cx, cy, cu, cv = seq(s[:, 0]) / m, seq(s[:, 1]) / m, seq(d[:, 0]) / m, seq(d[:, 1]) / m
        ex, ey, eu, ev = s[:, 0] - cx, s[:, 1] - cy, d[:, 0] - cu, d[:, 1] - cv
        ds, dd = seq(np.sqrt(ex * ex + ey * ey)) / m, seq(np.sqrt(eu * eu + ev * ev)) / m
        if not (np.isfinite(ds) and np.isfinite(dd)) or ds == 0.0 or dd == 0.0:
            return fail
        ss, sd = np.sqrt(2.0) / ds, np.sqrt(2.0) / dd
        M = np.zeros((9, 9))
        for x0, y0, u0, v0 in zip(s[:, 0], s[:, 1], d[:, 0], d[:, 1]):
            x, y, u, v = (x0 - cx) * ss, (y0 - cy) * ss, (u0 - cu) * sd, (v0 - cv) * sd
            r1 = np.array([-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u])
            r2 = np.array([0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v])
            M += np.outer(r1, r1) + np.outer(r2, r2)
        M = np.triu(M) + np.triu(M, 1).T
        lam, Q = jacobi(M)
        best = 0
        for c in range(1, 9):
            if lam[c] < lam[best]:
                best = c
        h = Q[:, best]
        A = np.zeros(9)
        for r in range(3):
            A[3 * r] = h[3 * r] * ss
            A[3 * r + 1] = h[3 * r + 1] * ss
            A[3 * r + 2] = (h[3 * r + 2] - A[3 * r] * cx) - A[3 * r + 1] * cy
        Hn = np.zeros(9)
        for c in range(3):
            Hn[c] = A[c] / sd + cu * A[6 + c]
            Hn[3 + c] = A[3 + c] / sd + cv * A[6 + c]
            Hn[6 + c] = A[6 + c]
        fro = 0.0
        for e in Hn:
            fro += e * e
        fro = np.sqrt(fro)
        if abs(Hn[8]) >= 1e-12 * fro:
            Hn = Hn / Hn[8]
        else:
            big = 0
            for e in range(1, 9):
                if abs(Hn[e]) > abs(Hn[big]):
                    big = e
            Hn = Hn / (-fro if Hn[big] < 0.0 else fro)
        det_n = det3(Hn)
        if not (np.isfinite(Hn).all() and np.isfinite(det_n) and abs(det_n) >= 1e-12):
            fail["stats"][3] = det_n
            return fail
        H = compose3(post, Hn.reshape(3, 3))
        Hinv = inverse3(H)
        err = np.full(n, np.nan)
        X, Y, w = apply3(H, s[:, 0], s[:, 1])
        U, V, t = apply3(post, d[:, 0], d[:, 1])
        dx, dy = X / w - U / t, Y / w - V / t
        e = np.sqrt(dx * dx + dy * dy)
        err[used] = e
        rms = np.sqrt(seq(e * e) / m)
        mx = np.nan if np.isnan(e).any() else e.max()
    return dict(H=H, Hinv=Hinv, err=err, stats=np.array([m, rms, mx, det_n]), status=True, Hn=Hn.reshape(3, 3))


def homography_exact4(src, dst):
    """the exact four-point homography with h22 = 1: the 8 x 8 linear system by np.linalg.solve"""
    A, b = [], []
    for (x, y), (u, v) in zip(np.asarray(src, np.float64), np.asarray(dst, np.float64)):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    return np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0).reshape(3, 3)


# ---- the perspective warp -------------------------------------------------------------------------------------------------
def warp_values(img, Hinv, out_size):
    """img uint8 [H, W, ch] -> the UNROUNDED float64 values [OH, OW, ch]; out_size = (width, height); Hinv maps output
    pixels to source positions.  A position outside (-1, W) x (-1, H), NaN included, gives 0; taps outside count 0."""
    img = np.asarray(img)
    H, W, ch = img.shape
    ow, oh = out_size
    u, v = np.meshgrid(np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64))
    X, Y, w = apply3(Hinv, u, v)
    with np.errstate(all="ignore"):
        su, sv = X / w, Y / w
        inside = (su > -1.0) & (su < W) & (sv > -1.0) & (sv < H)
    su, sv = np.where(inside, su, 0.0), np.where(inside, sv, 0.0)
    x0f, y0f = np.floor(su), np.floor(sv)
    a, b = (su - x0f)[..., None], (sv - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    pad = np.zeros((H + 2, W + 2, ch), np.float64)
    pad[1:-1, 1:-1] = img
    p00, p01 = pad[y0 + 1, x0 + 1], pad[y0 + 1, x0 + 2]
    p10, p11 = pad[y0 + 2, x0 + 1], pad[y0 + 2, x0 + 2]
    val = (1.0 - b) * ((1.0 - a) * p00 + a * p01) + b * ((1.0 - a) * p10 + a * p11)
    return np.where(inside[..., None], val, 0.0)


def warp_perspective(img, Hinv, out_size):
    return np.floor(warp_values(img, Hinv, out_size) + 0.5).astype(np.uint8)


# ---- the skeleton on the plan ---------------------------------------------------------------------------------------------
def wave_sum64(v):
    """the kernel's order: lane l adds its entries l, l + 64, .. in order, then the xor butterfly 32, 16, .. 1"""
    v = np.asarray(v, np.float64)
    lanes = np.zeros(64)
    for j, e in enumerate(v):
        lanes[j % 64] += e
    idx = np.arange(64)
    o = 32
    while o:
        lanes = lanes + lanes[idx ^ o]
        o >>= 1
    return lanes[0]


def project_world_to_bev_centered(kpts, center_world, center_px, mpp, use_axes=(0, 2), rot90_left=False):
    """one step: kpts [J, 3] -> (uv [J, 2], px int32 [J, 2], valid [J])"""
    kpts = np.asarray(kpts, np.float64)
    ax0, ax1 = use_axes
    cx, cz = center_world[ax0], center_world[ax1]
    cpx = np.asarray(center_px, np.float64)
    J = kpts.shape[0]
    uv, px, valid = np.full((J, 2), np.nan), np.zeros((J, 2), np.int32), np.zeros(J, bool)
    if not (np.isfinite(cx) and np.isfinite(cz) and np.isfinite(cpx).all()):
        return uv, px, valid
    u0, v0 = np.rint(cpx[0]), np.rint(cpx[1])
    for j in range(J):
        if not np.isfinite(kpts[j]).all():
            continue
        dx, dz = kpts[j, ax0] - cx, kpts[j, ax1] - cz
        if rot90_left:
            dx, dz = dz, dx
        du, dv = dx / mpp, -dz / mpp
        uv[j] = (u0 + du, v0 + dv)
        px[j] = np.rint(uv[j]).astype(np.int32)
        valid[j] = True
    return uv, px, valid


def bev_skeleton(X, center_px, mpp=0.02, use_axes=(0, 2), rot90_left=False):
    """X [T, J, 3], center_px [T, 2] -> (uv, px, valid, center_world)"""
    X = np.asarray(X, np.float64)
    T, J = X.shape[:2]
    uv, px, valid, cw = np.zeros((T, J, 2)), np.zeros((T, J, 2), np.int32), np.zeros((T, J), bool), np.zeros((T, 3))
    for t in range(T):
        for a in range(3):
            col = X[t, :, a]
            keep = ~np.isnan(col)
            with np.errstate(all="ignore"):
                cw[t, a] = wave_sum64(np.where(keep, col, 0.0)) / keep.sum() if keep.any() else np.nan
        uv[t], px[t], valid[t] = project_world_to_bev_centered(X[t], cw[t], center_px[t], mpp, use_axes, rot90_left)
    return uv, px, valid, cw


# ---- the ground track -----------------------------------------------------------------------------------------------------
def ground_track(p, fps):
    """p [P, T, 2] -> [P, T, 6] = step, path, vx, vy, speed, heading"""
    p = np.asarray(p, np.float64)
    P, T = p.shape[:2]
    out = np.full((P, T, 6), np.nan)
    fin = np.isfinite(p).all(-1)
    with np.errstate(all="ignore"):
        for k in range(P):
            path = 0.0
            for t in range(T):
                if t == 0:
                    step = 0.0
                elif fin[k, t] and fin[k, t - 1]:
                    d = p[k, t] - p[k, t - 1]
                    step = np.sqrt(d[0] * d[0] + d[1] * d[1])
                else:
                    step = np.nan
                if np.isfinite(step):
                    path += step
                out[k, t, 0], out[k, t, 1] = step, path
                if T > 1:
                    lo, hi = max(t - 1, 0), min(t + 1, T - 1)
                    if fin[k, lo] and fin[k, hi]:
                        v = (p[k, hi] - p[k, lo]) * fps
                        if hi - lo == 2:
                            v = v / 2.0
                        out[k, t, 2:4] = v
                vx, vy = out[k, t, 2], out[k, t, 3]
                out[k, t, 4] = np.sqrt(vx * vx + vy * vy)
                out[k, t, 5] = np.arctan2(vx, vy)
    return out


# ---- the chain of bev.process_front_clip ------------------------------------------------------------------------------------
def process_front_clip(frames, boxes_xywh, img_pts=None, calib_size=(1080, 1920), fps=30.0, skeleton=None, canvas=None):
    """frames uint8 [T, h, w, 3], boxes [T, N, 4] -> dict; the frame is sampled ONCE, with the inverse of the fit of the
    ground points carried into the frame's own pixels by A, the pixel-centre scaling of the reference's resize to calib_size"""
    frames = np.asarray(frames)
    T, h, w = frames.shape[:3]
    Hc, Wc = calib_size
    size, S = make_bev_canvas(**(canvas or {}))
    img_pts = DEFAULT_IMG_PTS if img_pts is None else np.asarray(img_pts, np.float32).astype(np.float64)
    foot_uv = foot_from_bbox_xyxy(unnormalize_bbox(convert_xywh_to_xyxy(np.asarray(boxes_xywh, np.float64)), (Hc, Wc)))
    fit = homography_fit(img_pts, DEFAULT_BEV_PTS_M, S)
    H_px, H_m = fit["H"], fit["Hn"]
    foot_px, foot_m = homography_points(foot_uv, H_px), homography_points(foot_uv, H_m)
    sx, sy = w / Wc, h / Hc
    own = img_pts if (h, w) == (Hc, Wc) else (img_pts + 0.5) * np.array([sx, sy]) - 0.5
    G = homography_fit(own, DEFAULT_BEV_PTS_M, S)["Hinv"]
    values = np.stack([warp_values(f, G, size) for f in frames])
    out = dict(values=values, bev=np.floor(values + 0.5).astype(np.uint8), foot_uv=foot_uv, foot_px=foot_px, foot_m=foot_m,
               track=ground_track(np.transpose(foot_m, (1, 0, 2)), fps), H_px=H_px, H_m=H_m, status=fit["status"])
    if skeleton is not None:
        out["skeleton"] = bev_skeleton(skeleton, foot_px[:, -1], 0.02, (0, 2), True)
    return out
