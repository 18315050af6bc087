"""Float64 NumPy restatement of the person origin, the camera update and the triangulation triage (DESIGN §2 "Person
origin", "Triage"), written from the rules and the reference's cited lines, not from the kernels:

    person_origin    vggt/multi_view_process.py:356-395 (extract_person_points) + :195-199 (the mean)
    recenter         :201-217
    triage           vggt/reproject.py:108-144, :334-341; triangulation/postprocess.py:38-43, :102-121 (two views -> V)
    step_chain       the per-step chain of infer.process_multi_view_clip(boxes=..., triage=True)
"""
from __future__ import annotations

import warnings

import numpy as np


def crop(box, map_hw, source_hw):
    """the box in map pixels -> (x1, y1, x2, y2), or None for an empty range or a non-finite corner"""
    H, W = map_hw
    src_h, src_w = source_hw
    b = [float(v) for v in box]
    if not all(np.isfinite(b)):
        return None
    sx, sy = W / src_w, H / src_h
    x1, x2, y1, y2 = int(b[0] * sx), int(b[2] * sx), int(b[1] * sy), int(b[3] * sy)
    x1, x2 = min(max(x1, 0), W - 1), min(max(x2, 0), W)
    y1, y2 = min(max(y1, 0), H - 1), min(max(y2, 0), H)
    if x2 <= x1 or y2 <= y1:
        return None
    return x1, y1, x2, y2


def person_origin(pointmap, box, source_hw):
    """pointmap [H, W, 3] float32 -> dict(n_box, n_valid, n_kept, median, std, origin [3], kept mask over the valid
    points, z of the valid points); every statistic in float64"""
    nan = float("nan")
    out = dict(n_box=0, n_valid=0, n_kept=0, median=nan, std=nan, origin=np.full(3, nan), kept=np.zeros(0, bool),
               z=np.zeros(0))
    c = crop(box, pointmap.shape[:2], source_hw)
    if c is None:
        return out
    x1, y1, x2, y2 = c
    P = np.asarray(pointmap)[y1:y2, x1:x2, :].reshape(-1, 3)
    out["n_box"] = len(P)
    P = P[np.isfinite(P).all(axis=1)].astype(np.float64)
    out["n_valid"] = n = len(P)
    if n == 0:
        return out
    z = np.sort(P[:, 2])
    median = z[n // 2] if n % 2 else (z[n // 2 - 1] + z[n // 2]) / 2.0
    mean = P[:, 2].sum() / n
    std = float(np.sqrt(((P[:, 2] - mean) ** 2).sum() / n))
    kept = np.abs(P[:, 2] - median) < 3.0 * std
    nk = int(kept.sum())
    out.update(median=float(median), std=std, n_kept=nk, kept=kept, z=P[:, 2])
    if nk:
        out["origin"] = P[kept].sum(axis=0) / nk
    return out


def margin(res):
    """the smallest | |z - median| - 3 std | over the valid points, in units of std (inf without a valid point or at
    std = 0, where nothing is kept whatever the rounding): a kept set can differ between two correct implementations
    only through a point for which this is tiny"""
    if res["n_valid"] == 0 or not res["std"] > 0:
        return float("inf")
    return float(np.abs(np.abs(res["z"] - res["median"]) - 3.0 * res["std"]).min() / res["std"])


def recenter(origins, n_kept, R, t):
    """origins [S, 3], n_kept [S], R [S, 3, 3], t [S, 3] (float64) -> origin [3], R', t' of multi_view_process.py:195-217:
    origin = mean of the views' origins in view order (zero if a view kept nothing); t_c += R_c origin; at S = 2 view 1
    is turned by diag(-1, 1, -1) and its t turned and then mirrored back in x and z."""
    S = len(R)
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    if all(int(k) > 0 for k in n_kept):
        acc = np.zeros(3)
        for v in range(S):
            acc = acc + np.asarray(origins[v], np.float64)
        origin = acc / S
    else:
        origin = np.zeros(3)
    for v in range(S):
        t[v] = t[v] + R[v] @ origin
    if S == 2:
        A = np.diag([-1.0, 1.0, -1.0])
        R[1] = A @ R[1]
        t[1] = A @ t[1]
        t[1][0] = -t[1][0]
        t[1][2] = -t[1][2]
    return origin, R, t


def triage(K, R, t, kp, X, conf=None, conf_thr=0.3, err_thresh_px=2.0):
    """K, R [T, V, 3, 3], t [T, V, 3], kp [T, V, J, 2], X [T, J, 3] (the triangulated joints), conf [T, V, J] | None ->
    dict(err [T, V, J], depth [T, V, J], em [T, J], pos [T, J], keep [T, J], X_clean, view_stats [T, V, 4], report [T, 5])"""
    K, R, t, kp, X = (np.asarray(a, np.float64) for a in (K, R, t, kp, X))
    T, V, J = kp.shape[:3]
    err, depth = np.empty((T, V, J)), np.empty((T, V, J))
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(T):
            for v in range(V):
                cam = X[i] @ R[i, v].T + t[i, v]          # [J, 3]
                xh = cam @ K[i, v].T
                depth[i, v] = xh[:, 2]
                err[i, v] = np.linalg.norm(xh[:, :2] / xh[:, 2:3] - kp[i, v], axis=1)
        em = err.sum(axis=1) / V
        pos = (depth > 0).all(axis=1)
        keep = pos & np.isfinite(em) & (em <= err_thresh_px)
        if conf is not None:
            keep &= (np.asarray(conf, np.float64) >= conf_thr).all(axis=1)
        X_clean = X.copy()
        X_clean[~keep] = np.nan
        view_stats = np.stack([np.sqrt(np.nanmean(err ** 2, axis=2)), np.nanmean(err, axis=2), np.nanmedian(err, axis=2),
                               np.nanmax(err, axis=2)], axis=-1)
        report = np.stack([np.sqrt(np.nanmean(em ** 2, axis=1)), np.nanmedian(em, axis=1), pos.mean(axis=1),
                           keep.mean(axis=1), keep.sum(axis=1).astype(np.float64)], axis=-1)
    return dict(err=err, depth=depth, em=em, pos=pos, keep=keep, X_clean=X_clean, view_stats=view_stats, report=report)


def reproject_two_views(K, R_rel, t_rel, kp, X):
    """vggt/reproject.py:108-144 written out for one step of two views without distortion: view 0 through K_0 [I | 0],
    view 1 through K_1 [R_rel | t_rel] -> err [2, J]"""
    K, kp, X = (np.asarray(a, np.float64) for a in (K, kp, X))
    p0 = X @ K[0].T
    p1 = (X @ np.asarray(R_rel, np.float64).T + np.asarray(t_rel, np.float64)) @ K[1].T
    return np.stack([np.linalg.norm(p0[:, :2] / p0[:, 2:3] - kp[0], axis=1),
                     np.linalg.norm(p1[:, :2] / p1[:, 2:3] - kp[1], axis=1)])


def unproject(depth, E, K):
    """vggt/vggt/utils/geometry.py:47-117 in float64: depth [H, W], E [3, 4], K [3, 3] -> world points [H, W, 3]"""
    depth, E, K = (np.asarray(a, np.float64) for a in (depth, E, K))
    H, W = depth.shape
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cam = np.stack([(u - K[0, 2]) * depth / K[0, 0], (v - K[1, 2]) * depth / K[1, 1], depth], axis=-1)
    return (cam - E[:, 3]) @ E[:, :3]          # R^T (cam - t)


def step_chain(point_maps, boxes, source_hw, E, K, kp, X, conf=None, conf_thr=0.3, err_thresh_px=2.0, cameras=None):
    """One time step after the model call: point_maps [S, H, W, 3] float32 (the device's unprojection), boxes [S, 4],
    E [S, 3, 4], K [S, 3, 3], kp [S, J, 2], X [J, 3] (the joints the device triangulated with the recentred cameras) ->
    dict(origin, R, t, stats, triage) with R, t rounded to float32 as the cameras that feed the triangulation are.
    `cameras` = (R, t) float32: the triage is evaluated through these instead (the device's own rounding of R, t, once
    the caller has compared it with the restated one: a last-bit difference in a camera moves an error by far more than
    the bound on the errors allows)."""
    S = len(point_maps)
    po = [person_origin(point_maps[v], boxes[v], source_hw) for v in range(S)]
    E = np.asarray(E, np.float64)
    origin, R, t = recenter([p["origin"] for p in po], [p["n_kept"] for p in po], E[:, :, :3], E[:, :, 3])
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    Rc, tc = (R32, t32) if cameras is None else cameras
    tri = triage(np.asarray(K)[None], np.asarray(Rc)[None], np.asarray(tc)[None], np.asarray(kp)[None], np.asarray(X)[None],
                 None if conf is None else np.asarray(conf)[None], conf_thr, err_thresh_px)
    return dict(origin=origin, R=R32, t=t32, stats=po, triage=tri)
