"""NumPy float64 restatement of the scene cloud's rules (DESIGN §2 "Scene cloud"; include/skimi.h, skimi_scene_cloud):
what predictions_to_glb (vggt/visual_util.py:39-236) computes for one time step, with every percentile taken in float64
on the sorted values.  Sort-based, one scene at a time, no cleverness: this is what the kernels are tested against."""
import numpy as np


def key_of(x):
    """the order-preserving 32-bit key of float32 values (-0.0 just below +0.0, +-inf ordered)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def colour_u8(v):
    """rule 2: (uint8)(float32(v) * 255), truncated toward zero; NaN -> 0, below 0 -> 0, >= 256 -> 255"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(v, np.float32) * np.float32(255.0)
        out = np.zeros(p.shape, np.uint8)
        mid = (p >= 0) & (p < 256)
        out[mid] = np.trunc(p[mid]).astype(np.uint8)
        out[p >= 256] = 255
    return out


def percentile_linear(values, q):
    """rule 3: NumPy's `linear` percentile of float32 values in float64 on the exact order statistics -> (value, lo, hi);
    NaN x 3 if a value is NaN"""
    x = np.asarray(values, np.float32).reshape(-1)
    m = x.size
    if np.isnan(x).any():
        return np.nan, np.nan, np.nan
    s = x[np.argsort(key_of(x), kind="stable")].astype(np.float64)
    v = q / 100.0 * (m - 1)
    i = int(np.floor(v))
    g = v - i
    lo, hi = s[i], s[min(i + 1, m - 1)]
    with np.errstate(invalid="ignore"):
        d = hi - lo
        val = lo + d * g if g < 0.5 else hi - d * (1.0 - g)
    return float(val), float(lo), float(hi)


def alignment(extrinsic):
    """rule 7: A = E0^-1 diag(-1, -1, 1, 1), a general 4 x 4 inverse in float64"""
    E = np.eye(4)
    E[:3, :4] = np.asarray(extrinsic, np.float32)[0].astype(np.float64)
    return np.linalg.inv(E) @ np.diag([-1.0, -1.0, 1.0, 1.0])


def scene_cloud(points, conf, images, extrinsic, conf_thres=50.0, mask_black_bg=False, mask_white_bg=False, align=True,
                capacity=None):
    """One scene: points [S, H, W, 3], conf [S, H, W], images [S, 3, H, W] or [S, H, W, 3], extrinsic [S, 3, 4], float32.
    -> dict(xyz, rgb (the first min(count, capacity) kept rows), count, threshold, lo, hi, lower, upper, scale, transform,
    n_nan_conf, n_nonfinite, mask)"""
    points = np.asarray(points, np.float32)
    conf = np.asarray(conf, np.float32).reshape(-1)
    images = np.asarray(images, np.float32)
    if not 0.0 <= conf_thres <= 100.0:
        raise ValueError("conf_thres is a percentile in [0, 100]")
    n = conf.size
    P = points.reshape(-1, 3)
    if images.ndim == 4 and images.shape[1] == 3:
        images = np.transpose(images, (0, 2, 3, 1))
    rgb = colour_u8(images.reshape(-1, 3))
    thr, lo, hi = percentile_linear(conf, conf_thres)
    if conf_thres == 0.0:
        thr = 0.0
    with np.errstate(invalid="ignore"):
        mask = (conf.astype(np.float64) >= thr) & (conf > np.float32(1e-5))
    if mask_black_bg:
        mask &= rgb.astype(np.int64).sum(axis=1) >= 16
    if mask_white_bg:
        mask &= ~((rgb[:, 0] > 240) & (rgb[:, 1] > 240) & (rgb[:, 2] > 240))
    kept, kept_rgb = P[mask], rgb[mask]
    count = int(mask.sum())
    lower, upper = np.full(3, np.nan), np.full(3, np.nan)
    if count == 0:
        scale = 1.0
    else:
        for a in range(3):
            lower[a] = percentile_linear(kept[:, a], 5.0)[0]
            upper[a] = percentile_linear(kept[:, a], 95.0)[0]
        with np.errstate(invalid="ignore", over="ignore"):
            d = upper - lower
            scale = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    A = alignment(extrinsic)
    cap = n if capacity is None else int(capacity)
    xyz = kept[:cap]
    if align:
        with np.errstate(invalid="ignore", over="ignore"):
            xyz = (xyz.astype(np.float64) @ A[:3, :3].T + A[:3, 3]).astype(np.float32)
    return dict(xyz=xyz, rgb=kept_rgb[:cap], count=count, threshold=thr, lo=lo, hi=hi, lower=lower, upper=upper, scale=scale,
                transform=A, n_nan_conf=int(np.isnan(conf).sum()), n_nonfinite=int((~np.isfinite(kept).all(axis=1)).sum()),
                mask=mask)
