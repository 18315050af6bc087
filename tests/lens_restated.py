"""NumPy float64 restatement of the lens model (DESIGN §2 "Lens distortion"), written from OpenCV's documented formulas:
the rational + tangential + thin-prism model, its fixed-point inverse with a fixed iteration count, cv2.projectPoints
with rotation matrices, and the on-the-fly bilinear frame warp.  Every expression is evaluated in the order csrc/lens.hip
evaluates it (no fused multiply-add on either side), so the two agree to the last bit where the tests ask for it.

K, P and new_K are read as (fx, fy, cx, cy) = ([0,0], [1,1], [0,2], [1,2]): skew and the third row are not part of the
model, as in cv2's distortion code.  dist: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (tx ty), zero-padded from 4, 5, 8, 12 or 14.
"""
import numpy as np

COEFF_COUNTS = (4, 5, 8, 12, 14)


def pad_dist(dist):
    """[..., k] with k in COEFF_COUNTS -> float64 [..., 12]; a non-zero tilt coefficient is refused"""
    d = np.asarray(dist, np.float64)
    if d.shape[-1] not in COEFF_COUNTS:
        raise ValueError(f"{d.shape[-1]} distortion coefficients: OpenCV's vectors hold 4, 5, 8, 12 or 14")
    if d.shape[-1] == 14:
        if np.any(d[..., 12:] != 0):
            raise ValueError("the tilt model (tx, ty) is not supported")
        d = d[..., :12]
    out = np.zeros(d.shape[:-1] + (12,), np.float64)
    out[..., :d.shape[-1]] = d
    return out


def _fc(K):
    K = np.asarray(K, np.float64)
    return K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2]


def _tangential(x, y, r2, r4, d):
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = d
    a = (2.0 * x) * y
    dx = p1 * a + p2 * (r2 + (2.0 * x) * x) + s1 * r2 + s2 * r4
    dy = p1 * (r2 + (2.0 * y) * y) + p2 * a + s3 * r2 + s4 * r4
    return dx, dy


def _radial(r2, r4, d):
    """-> (numerator, denominator) of c"""
    r6 = r4 * r2
    return 1.0 + d[0] * r2 + d[1] * r4 + d[4] * r6, 1.0 + d[5] * r2 + d[6] * r4 + d[7] * r6


def distort_normalized(x, y, dist):
    """the forward model on normalised coordinates; dist [12] (or broadcastable [12, ...] columns)"""
    d = [np.asarray(v, np.float64) for v in np.moveaxis(pad_dist(dist), -1, 0)]
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        r4 = r2 * r2
        num, den = _radial(r2, r4, d)
        c = num / den
        dx, dy = _tangential(x, y, r2, r4, d)
        return x * c + dx, y * c + dy


def undistort_normalized(xd, yd, dist, iters=20):
    """OpenCV's fixed-point inverse, exactly `iters` rounds: x <- (x_d - tangential(x)) * (den / num)(x)"""
    d = [np.asarray(v, np.float64) for v in np.moveaxis(pad_dist(dist), -1, 0)]
    xd, yd = np.asarray(xd, np.float64), np.asarray(yd, np.float64)
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            r2 = x * x + y * y
            r4 = r2 * r2
            num, den = _radial(r2, r4, d)
            ic = den / num
            dx, dy = _tangential(x, y, r2, r4, d)
            x, y = (xd - dx) * ic, (yd - dy) * ic
    return x, y


def distort_points(x, K, dist, P=None, normalized=False):
    """undistorted points [..., 2] (pixels of P, default K; or normalised) -> distorted pixels of K"""
    x = np.asarray(x, np.float64)
    fx, fy, cx, cy = _fc(K)
    if normalized:
        xn, yn = x[..., 0], x[..., 1]
    else:
        pfx, pfy, pcx, pcy = _fc(K if P is None else P)
        xn, yn = (x[..., 0] - pcx) / pfx, (x[..., 1] - pcy) / pfy
    xd, yd = distort_normalized(xn, yn, dist)
    return np.stack([fx * xd + cx, fy * yd + cy], -1)


def undistort_points(x, K, dist, P=None, iters=20, normalized=False):
    """distorted pixels [..., 2] of K -> (undistorted points as pixels of P (default K) or normalised, resid_px [...]).
    resid_px = the distance in pixels of K between the input and the re-distorted result; a non-finite point or residual
    makes both NaN."""
    x = np.asarray(x, np.float64)
    fx, fy, cx, cy = _fc(K)
    with np.errstate(all="ignore"):
        xd, yd = (x[..., 0] - cx) / fx, (x[..., 1] - cy) / fy
        xu, yu = undistort_normalized(xd, yd, dist, iters)
        xr, yr = distort_normalized(xu, yu, dist)
        du, dv = fx * (xr - xd), fy * (yr - yd)
        resid = np.sqrt(du * du + dv * dv)
        if normalized:
            ox, oy = xu, yu
        else:
            pfx, pfy, pcx, pcy = _fc(K if P is None else P)
            ox, oy = pfx * xu + pcx, pfy * yu + pcy
    bad = ~(np.isfinite(ox) & np.isfinite(oy) & np.isfinite(resid))
    out = np.stack([np.where(bad, np.nan, ox), np.where(bad, np.nan, oy)], -1)
    return out, np.where(bad, np.nan, resid)


def project_points(X, R, t, K, dist=None):
    """cv2.projectPoints with a rotation matrix: X [n, 3], R [3, 3], t [3] -> (pixels [n, 2], camera-frame depth [n])"""
    X, R, t = np.asarray(X, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64)
    fx, fy, cx, cy = _fc(K)
    with np.errstate(all="ignore"):
        Xc = [R[i, 0] * X[..., 0] + R[i, 1] * X[..., 1] + R[i, 2] * X[..., 2] + t[i] for i in range(3)]
        xn, yn = Xc[0] / Xc[2], Xc[1] / Xc[2]
        xd, yd = distort_normalized(xn, yn, np.zeros(12) if dist is None else dist)
        return np.stack([fx * xd + cx, fy * yd + cy], -1), Xc[2]


def source_positions(K, dist, new_K, out_w, out_h):
    """(su, sv) [out_h, out_w]: where output pixel (u, v) samples the source frame"""
    fx, fy, cx, cy = _fc(K)
    nfx, nfy, ncx, ncy = _fc(new_K)
    u, v = np.meshgrid(np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64))
    xd, yd = distort_normalized((u - ncx) / nfx, (v - ncy) / nfy, dist)
    return fx * xd + cx, fy * yd + cy


def undistort_image_values(img, K, dist, new_K=None, out_size=None):
    """img uint8 [H, W, ch] -> the UNROUNDED float64 values [OH, OW, ch] of the warp (out_size = (width, height)).
    Taps outside the source are 0 (constant border); a source position that is not inside (-1, W) x (-1, H), NaN
    included, gives 0."""
    img = np.asarray(img)
    H, W, ch = img.shape
    ow, oh = (W, H) if out_size is None else out_size
    su, sv = source_positions(K, dist, K if new_K is None else new_K, ow, oh)
    with np.errstate(all="ignore"):
        inside = (su > -1.0) & (su < W) & (sv > -1.0) & (sv < H)
    su, sv = np.where(inside, su, 0.0), np.where(inside, sv, 0.0)
    x0f, y0f = np.floor(su), np.floor(sv)
    a, b = (su - x0f)[..., None], (sv - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    pad = np.zeros((H + 2, W + 2, ch), np.float64)   # one zero pixel all round: the constant border
    pad[1:-1, 1:-1] = img
    p00, p01 = pad[y0 + 1, x0 + 1], pad[y0 + 1, x0 + 2]
    p10, p11 = pad[y0 + 2, x0 + 1], pad[y0 + 2, x0 + 2]
    val = (1.0 - b) * ((1.0 - a) * p00 + a * p01) + b * ((1.0 - a) * p10 + a * p11)
    return np.where(inside[..., None], val, 0.0)


def undistort_image(img, K, dist, new_K=None, out_size=None):
    """-> uint8 [OH, OW, ch] = floor(value + 0.5)"""
    return np.floor(undistort_image_values(img, K, dist, new_K, out_size) + 0.5).astype(np.uint8)


def near_tie(values, eps=1e-6):
    """bool mask of the unrounded values within eps of k + 0.5, where a last-bit difference may flip the rounding"""
    f = values - np.floor(values)
    return np.abs(f - 0.5) <= eps

