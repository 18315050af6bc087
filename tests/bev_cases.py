"""Seeded inputs of the bird's-eye-view tests (tests/test_bev_cpu.py, tests/test_bev_gpu.py, tools/make_goldens.py bev,
tools/mb_bev.py)."""
import numpy as np

DEFAULT_IMG_PTS = np.array([[0.0, 1080.0], [1920.0, 1080.0], [1336.0, 130.0], [600.0, 130.0]])
DEFAULT_BEV_PTS_M = np.array([[-15.0, 0.0], [15.0, 0.0], [15.0, 60.0], [-15.0, 60.0]])
# the default geometry's own matrix, pixels -> metres, to three digits: the "truth" the noisy fits are drawn from
TRUE_H = np.array([[0.0479, 0.0403, -46.0], [0.0, -0.1856, 200.4], [0.0, 0.00268, 1.0]])

FIT_NOISY_COUNTS = (5, 64, 65, 1100)
POINT_COUNTS = (1, 63, 65, 17 * 243)
N_QUADS = 50

# (C, F, H, W, OH, OW, ch, per_frame)
WARP_CASES = {
    "ragged_rgb": (1, 1, 61, 97, 45, 83, 3, False),        # unaligned rows, ragged end
    "per_camera_grey": (2, 3, 33, 70, 31, 66, 1, False),   # a matrix per camera
    "per_frame_rgba": (1, 2, 40, 50, 37, 129, 4, True),    # a matrix per frame
    "two_blocks_half_out": (1, 1, 61, 97, 9, 257, 3, False),   # two blocks across, half the output outside the source
    "dword_rgb": (1, 1, 61, 97, 45, 84, 3, False),         # the dword path
}


def _proj(H, x):
    p = np.concatenate([x, np.ones((len(x), 1))], 1) @ H.T
    return p[:, :2] / p[:, 2:3]


def generic_quad(seed):
    """a jittered rectangle of a 1920 x 1080 frame -> a jittered rectangle in metres: both convex, no three collinear"""
    rng = np.random.default_rng(1000 + seed)
    base = np.array([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0], [0.0, 0.0]])
    src = (base * 0.6 + 0.2 + rng.uniform(-0.15, 0.15, (4, 2))) * [1920.0, 1080.0]
    dst = (base * 0.6 + 0.2 + rng.uniform(-0.15, 0.15, (4, 2))) * [40.0, 80.0] - [20.0, 10.0]
    return src, dst


def noisy_fit(n, seed=0):
    """n ground points seen through TRUE_H, the image points with 0.5 px of noise"""
    rng = np.random.default_rng(2000 + 7 * n + seed)
    src = rng.uniform([100.0, 200.0], [1820.0, 1060.0], (n, 2))
    dst = _proj(TRUE_H, src)
    return src + rng.normal(scale=0.5, size=src.shape), dst


def collinear4():
    src = np.array([[100.0, 100.0], [300.0, 200.0], [500.0, 300.0], [900.0, 500.0]])
    return src, np.array([[0.0, 0.0], [2.0, 1.0], [4.0, 2.0], [8.0, 4.0]])


def points_case(n, G=3, seed=0):
    """G groups of n image points and a matrix each (perturbations of TRUE_H composed with the canvas scale)"""
    rng = np.random.default_rng(3000 + n + seed)
    x = rng.uniform([0.0, 150.0], [1920.0, 1080.0], (G, n, 2))
    H = np.stack([TRUE_H * (1.0 + 0.05 * rng.standard_normal((3, 3))) for _ in range(G)])
    return x, H


def warp_case(name):
    """-> (frames uint8 [C, F, H, W, ch], Hinv [C, 3, 3] or [C, F, 3, 3], (OW, OH), per_frame): generic perspective maps whose
    source positions cover the frame and leave it on some sides"""
    C, F, H, W, OH, OW, ch, per_frame = WARP_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    frames = rng.integers(0, 256, (C, F, H, W, ch), dtype=np.uint8)
    mats = []
    for _ in range(C * F if per_frame else C):
        span = 2.0 if name == "two_blocks_half_out" else 1.15
        sx, sy = span * W / OW, 1.15 * H / OH
        th = rng.uniform(-0.08, 0.08)
        g = np.array([[sx * np.cos(th), -sy * np.sin(th), rng.uniform(-0.1, 0.0) * W],
                      [sx * np.sin(th), sy * np.cos(th), rng.uniform(-0.1, 0.0) * H],
                      [rng.uniform(-0.3, 0.3) / OW, rng.uniform(-0.3, 0.3) / OH, 1.0]])
        mats.append(g * rng.uniform(0.5, 2.0))      # a homography's scale is free
    Hinv = np.stack(mats).reshape((C, F, 3, 3) if per_frame else (C, 3, 3))
    return frames, Hinv, (OW, OH), per_frame


def frame_matrix(Hinv, per_frame, c, f):
    return Hinv[c, f] if per_frame else Hinv[c]


def skeleton_case(T, J, seed=0):
    """world joints [T, J, 3] with NaN joints, a NaN coordinate, an all-NaN step (T > 2) and centre pixels [T, 2]"""
    rng = np.random.default_rng(4000 + 31 * T + J + seed)
    X = rng.normal(size=(T, J, 3)) * [0.3, 0.8, 0.3] + [1.0, 0.9, 6.0] + np.cumsum(rng.normal(scale=0.05, size=(T, 1, 3)), 0)
    X[0, 3] = np.nan
    X[T - 1, J - 1, 1] = np.nan
    if T > 2:
        X[T // 2] = np.nan
        X[1, :, 1] = np.nan              # a whole column: the step's centre has a NaN the plan does not use
    center_px = rng.uniform([100.0, 200.0], [700.0, 1500.0], (T, 2))
    if T > 2:
        center_px[2, 0] = 350.5          # rint of the centre pixel itself at a half
    return X, center_px


def halfway_case(J=17, seed=0):
    """joints on a 1/8 m grid whose mean is exactly 0 and 0.25 m per pixel: every shift is a multiple of 0.5 px, so the
    rounding meets exact halves on both sides of zero -> (X [2, J, 3], center_px [2, 2], metres_per_pixel)"""
    rng = np.random.default_rng(5000 + J + seed)
    X = rng.integers(-40, 41, (2, J, 3)).astype(np.float64) / 8.0
    X[1, 2] = np.nan                      # a NaN joint: the mean runs over the others
    X[:, J - 1] = -np.nansum(X[:, :J - 1], 1)
    return X, np.array([[400.0, 800.0], [401.0, 799.0]]), 0.25


def track_case(P, T, seed=0):
    """P tracks of T ground positions in metres with gaps"""
    rng = np.random.default_rng(6000 + 13 * T + P + seed)
    t = np.arange(T)[None, :, None] / 30.0
    p = np.concatenate([3.0 * np.sin(1.3 * t + rng.uniform(0, 3, (P, 1, 1))), 50.0 - 9.0 * t + 0 * rng.uniform(size=(P, 1, 1))], -1)
    p = p + rng.normal(scale=0.02, size=p.shape)
    if T >= 2:
        p[0, T - 1, 0] = np.nan
    if T > 20:
        p[0, 5] = np.nan
        p[P - 1, 9:12] = np.nan
        p[P - 1, 0] = np.inf
    return p


def front_clip_case(seed=0):
    """T = 3 frames of 54 x 96 RGB, two normalised xywh boxes a frame and side-view joints [3, 21, 3]"""
    rng = np.random.default_rng(7000 + seed)
    frames = rng.integers(0, 256, (3, 54, 96, 3), dtype=np.uint8)
    xy = rng.uniform(0.2, 0.6, (3, 2, 2))
    wh = rng.uniform(0.05, 0.3, (3, 2, 2))
    X, _ = skeleton_case(3, 21, seed)
    return frames, np.concatenate([xy, wh], -1), X
