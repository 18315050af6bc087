"""Seeded frames for the image-feature tests, made in NumPy: a rectangle-mosaic texture on two planes at different depths seen
by two pinhole cameras of known pose, and the frames that reach the code's edges.  The restated results are computed once
and shared (tests/features_restated.py, tests/essential_restated.py).

Truth bounds of the end-to-end pose (features -> cross-checked matches -> essential_ransac), measured with the restatement on
the CPU over PAIRS x TRUTH_SEEDS (tests/test_features_cpu.py::test_restated_chain_pose_and_match_quality prints them):
    worst rotation angle error            MEASURED_ROT_DEG
    worst translation-direction error     MEASURED_DIR_DEG
and the bounds are twice those, as the chessboard detector's truth bound was set.
"""
import functools

import numpy as np

import essential_restated as er
import features_restated as fr

W, H, FOCAL = 320, 240, 300.0
K = np.array([[FOCAL, 0.0, (W - 1) / 2.0], [0.0, FOCAL, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
Z_NEAR, Z_FAR = 4.0, 6.0
NEAR_BOX = (-3.0, -0.2, 0.4, 2.5)        # x1, y1, x2, y2 of the near plane's rectangle in world units
TEX_SCALE = 60.0                         # texture pixels per world unit: about one per image pixel
MAX_FEATURES, MAX_MATCHES, HYPOTHESES, SEED, BASELINE = 500, 256, 256, 7, 0.5
# (name, roll, yaw, pitch in degrees, t)
PAIRS = (("roll10", 10.0, 3.0, 0.0, (0.5, 0.0, 0.05)),
         ("roll-20_in", -20.0, 0.0, 2.0, (0.4, 0.1, 0.3)),
         ("roll25_out", 25.0, -2.0, 0.0, (-0.5, 0.05, -0.25)))
TRUTH_SEEDS = (0, 1, 2, 3)
MEASURED_ROT_DEG, MEASURED_DIR_DEG = 3.342, 11.297     # pair roll10 seed 3; pair roll25_out seed 2
ROT_BOUND_DEG, DIR_BOUND_DEG = 2 * MEASURED_ROT_DEG, 2 * MEASURED_DIR_DEG


def rot(roll, yaw, pitch):
    r, y, p = np.radians([roll, yaw, pitch])
    Rz = np.array([[np.cos(r), -np.sin(r), 0], [np.sin(r), np.cos(r), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(p), -np.sin(p)], [0, np.sin(p), np.cos(p)]])
    return Rz @ Ry @ Rx


def pair_pose(name):
    _, roll, yaw, pitch, t = next(p for p in PAIRS if p[0] == name)
    t = np.array(t, dtype=np.float64)
    return rot(roll, yaw, pitch), t


@functools.lru_cache(maxsize=None)
def texture(seed, size=768, rects=900):
    rng = np.random.default_rng(seed)
    t = np.full((size, size), 128, dtype=np.int64)
    for _ in range(rects):
        x0, y0 = rng.integers(0, size, 2)
        w, h = rng.integers(6, 70, 2)
        t[y0:y0 + h, x0:x0 + w] = rng.integers(16, 240)
    return t


def _sample(tex, X, Y):
    n = tex.shape[0]
    u, v = X * TEX_SCALE + n / 2.0, Y * TEX_SCALE + n / 2.0
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    a, b = u - u0, v - v0
    g = lambda i, j: tex[np.mod(j, n), np.mod(i, n)]   # noqa: E731
    return (1 - b) * ((1 - a) * g(u0, v0) + a * g(u0 + 1, v0)) + b * ((1 - a) * g(u0, v0 + 1) + a * g(u0 + 1, v0 + 1))


def _hit(R, t, x, y):
    """the world points seen at pixels (x, y) of the camera X_c = R X_w + t, and whether they lie on the near plane"""
    d = np.stack([(x - K[0, 2]) / FOCAL, (y - K[1, 2]) / FOCAL, np.ones_like(x, dtype=np.float64)], axis=-1) @ R   # R^T d
    o = -R.T @ t
    out = np.zeros(d.shape)
    near = np.zeros(d.shape[:-1], dtype=bool)
    for z, first in ((Z_NEAR, True), (Z_FAR, False)):
        s = (z - o[2]) / d[..., 2]
        P = o + s[..., None] * d
        if first:
            near = (P[..., 0] >= NEAR_BOX[0]) & (P[..., 0] < NEAR_BOX[2]) & (P[..., 1] >= NEAR_BOX[1]) & (P[..., 1] < NEAR_BOX[3])
            out[near] = P[near]
        else:
            out[~near] = P[~near]
    return out, near


def render(R, t, seed, w=W, h=H):
    """uint8 [h, w]: the two planes with their textures and +-2 gray levels of noise"""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    P, near = _hit(R, t, x, y)
    img = np.where(near, _sample(texture(2 * seed + 1), P[..., 0], P[..., 1]), _sample(texture(2 * seed), P[..., 0], P[..., 1]))
    rng = np.random.default_rng(1000 + seed + int(1e6 * abs(t).sum()))
    return np.clip(np.rint(img) + rng.integers(-2, 3, img.shape), 0, 255).astype(np.uint8)


def true_match(R, t, xy):
    """where the scene points seen at xy [n, 2] of the first camera (identity pose) appear in the second"""
    P, _ = _hit(np.eye(3), np.zeros(3), xy[:, 0], xy[:, 1])
    Xc = P @ R.T + t
    return np.stack([FOCAL * Xc[:, 0] / Xc[:, 2] + K[0, 2], FOCAL * Xc[:, 1] / Xc[:, 2] + K[1, 2]], axis=1)


@functools.lru_cache(maxsize=None)
def view_pair(name, seed=0):
    """(frame1, frame2) uint8 [H, W] of a pair"""
    R, t = pair_pose(name)
    return render(np.eye(3), np.zeros(3), seed), render(R, t, seed)


def colour(gray_frame, ch, seed):
    """a 1, 3 or 4 channel frame whose B, G, R differ by a little noise (alpha: noise that must be ignored)"""
    if ch == 1:
        return gray_frame[:, :, None].copy()
    rng = np.random.default_rng(seed)
    f = np.clip(gray_frame[:, :, None].astype(np.int64) + rng.integers(-3, 4, gray_frame.shape + (3,)), 0, 255)
    if ch == 4:
        f = np.concatenate([f, rng.integers(0, 256, gray_frame.shape + (1,))], axis=2)
    return f.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frames():
    """name -> uint8 [h, w, ch]: the frames of the bitwise comparison"""
    out = {}
    for i, ((name, *_), ch) in enumerate(zip(PAIRS, (1, 3, 4))):
        a, b = view_pair(name, i)                        # another scene for every pair
        out[f"{name}_a_ch{ch}"], out[f"{name}_b_ch{ch}"] = colour(a, ch, 11), colour(b, ch, 12)
    out["crop_317x211"] = colour(view_pair(PAIRS[0][0])[0][7:218, 2:319], 3, 13)
    rng = np.random.default_rng(5)
    out["constant"] = np.full((H, W, 1), 97, dtype=np.uint8)
    out["noise"] = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    out["tiled"] = np.tile(rng.integers(0, 256, (40, 40, 1), dtype=np.uint8), (6, 8, 1))    # equal responses: the tie rule
    out["small_40x36"] = rng.integers(0, 256, (36, 40, 3), dtype=np.uint8)
    out["small_30x30"] = rng.integers(0, 256, (30, 30, 1), dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, max_features=MAX_FEATURES, levels=8, threshold=20):
    return fr.orb_features(frames()[name], max_features, levels, threshold)


def chain_inputs(f1, f2, max_features=MAX_FEATURES, max_matches=MAX_MATCHES):
    """restated features of two frames -> (matches, x2d [2, max_matches, 2] NaN-padded)"""
    a, b = fr.orb_features(f1, max_features), fr.orb_features(f2, max_features)
    pairs, dist, count = fr.match_hamming(a["desc"][:a["count"]], b["desc"][:b["count"]], True, None, None, max_matches)
    x2d = np.full((2, max_matches, 2), np.nan)
    x2d[0, :count], x2d[1, :count] = a["xy"][pairs[:count, 0]], b["xy"][pairs[:count, 1]]
    return (pairs, dist, count), x2d


def chain_pose(x2d, group_offset=0):
    return er.essential_ransac(x2d, np.stack([K, K]), group_size=x2d.shape[1], hypotheses=HYPOTHESES, seed=SEED,
                               group_offset=group_offset, baseline=BASELINE)


def pose_frames(name):
    """the pair as three-channel B, G, R frames with colour noise: frame PAIRS.index(name) of the pose clips"""
    a, b = view_pair(name, [p[0] for p in PAIRS].index(name))
    return colour(a, 3, 21), colour(b, 3, 22)


@functools.lru_cache(maxsize=None)
def restated_chain(name):
    """the restated chain on pose_frames(name) as frame f of the clip: (x2d, the restated essential_ransac result)"""
    _, x2d = chain_inputs(*pose_frames(name))
    return x2d, chain_pose(x2d, [p[0] for p in PAIRS].index(name))


def pose_errors(R, t, R_true, t_true):
    """(rotation angle, translation-direction angle) in degrees"""
    c = (np.trace(R_true.T @ R) - 1.0) / 2.0
    d = float(t.reshape(3) @ t_true) / (np.linalg.norm(t) * np.linalg.norm(t_true))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.degrees(np.arccos(np.clip(d, -1.0, 1.0))))
