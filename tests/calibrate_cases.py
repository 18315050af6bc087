"""Inputs of the calibration tests: corners synthesised from tests/golden/calibrate.npz (the camera matrix, the first eight
coefficients, the frame size and 24 board poses of the calibration the reference ships) by projecting the board and adding
seeded Gaussian noise.  The shapes are the smallest that reach every path of csrc/calibrate.hip: V = 3 (the minimum),
V = 6 and 8 (up to one view a wave), V = 12 and 24 (waves strided over the views; V n = 648 > 512 threads), a 10 x 7 board
(n = 70: two chunks of a wave), and the masks of rule 1."""
from pathlib import Path

import numpy as np

import calibrate_restated as cr

GOLD = Path(__file__).resolve().parent / "golden" / "calibrate.npz"


def fixture():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def prepare_object_points(board, square):
    """the reference's prepare_object_points without its float32 rounding and its z column"""
    cols, rows = board
    return np.mgrid[0:cols, 0:rows].T.reshape(-1, 2).astype(np.float64) * float(square)


def true_params():
    """the fixture's twelve parameters: the corners are always those of its full rational lens, whatever model is fitted
    (its first 4 or 5 coefficients alone describe no lens: 1 + k1 r^2 + k2 r^4 changes sign inside the frame)"""
    f = fixture()
    K = f["camera_matrix"]
    return np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], f["dist_coeffs"][:8]])


def rodrigues(w):
    import resect_restated as rr
    return rr.exp_so3(np.asarray(w, np.float64))


def corners(views, noise, seed, board=(9, 6)):
    """-> obj [n, 2], img [V, n, 2], the true parameters [12]"""
    f = fixture()
    obj = prepare_object_points(board, float(f["square"]))
    p = true_params()
    rng = np.random.default_rng(seed)
    img = np.stack([cr.project(p, rodrigues(f["rvecs"][v]), f["tvecs"][v], obj) for v in views])
    return obj, img + noise * rng.normal(0, 1, img.shape), p


MASKS = {4: cr.free_mask(names=("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")),
         5: cr.free_mask(rational_model=False),
         8: cr.free_mask(rational_model=True)}
SIZE = (1920, 1080)
SPREAD = {3: (0, 9, 20), 4: (0, 7, 13, 20), 6: (0, 4, 9, 13, 18, 22), 8: (0, 3, 6, 9, 12, 16, 19, 22),
          12: tuple(range(0, 24, 2)), 24: tuple(range(24))}


def case(name, V, n_coeffs, noise, seed, board=(9, 6), **kw):
    obj, img, p = corners(SPREAD[V], noise, seed, board)
    return name, dict(obj=obj, img=img, truth=p, rational=n_coeffs == 8), dict(dict(mask=MASKS[n_coeffs]), **kw)


def cases():
    """(name, data, keyword arguments of calibrate_camera)"""
    out = [case("V3_c4_n0.05", 3, 4, 0.05, 1), case("V6_c5_n0.1", 6, 5, 0.1, 2), case("V8_c5_n0.1", 8, 5, 0.1, 3),
           case("V12_c8_n0", 12, 8, 0.0, 4), case("V12_c8_n0.1", 12, 8, 0.1, 5), case("V24_c8_n0.1", 24, 8, 0.1, 6),
           case("V4_c5_board10x7", 4, 5, 0.1, 7, board=(10, 7))]
    # rule 1: a view with NaN corners, a view with 3 used corners (dropped), and the same with one more view switched off
    name, d, kw = case("V6_c5_masks", 6, 5, 0.1, 8)
    d["img"][1, 5] = np.nan
    d["img"][2, 17, 0] = np.inf
    d["img"][4, 3:] = np.nan
    out.append((name, d, kw))
    # G = 5 masks over 8 views: all, one off, leave-two-out, 3 views (the minimum) and 2 views (fails)
    name, d, kw = case("V8_c5_G5", 8, 5, 0.1, 9)
    use = np.ones((5, 8), np.uint8)
    use[1, 3] = 0
    use[2, [0, 7]] = 0
    use[3] = [1, 0, 0, 1, 0, 0, 1, 0]
    use[4] = [0, 0, 1, 0, 0, 1, 0, 0]
    out.append((name, d, dict(kw, use=use)))
    # K0 / dist0 given (cv2's USE_INTRINSIC_GUESS): the truth moved by 2 %
    name, d, kw = case("V6_c5_K0", 6, 5, 0.1, 10)
    p = d["truth"] * np.array([1.02, 0.98, 1.01, 0.99] + [1.0] * 8)
    K0 = np.array([[[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1.0]]])
    out.append((name, d, dict(kw, K0=K0, dist0=np.concatenate([0.5 * p[4:], np.zeros(4)])[None])))
    # fixed principal point; zero tangential
    name, d, kw = case("V6_c5_fixed_pp", 6, 5, 0.1, 11)
    out.append((name, d, dict(kw, mask=kw["mask"] & ~0b1100)))
    name, d, kw = case("V6_c5_zero_tangent", 6, 5, 0.1, 12)
    out.append((name, d, dict(kw, mask=cr.free_mask(rational_model=False, zero_tangent=True))))
    return out


def run(d, kw, **over):
    return cr.calibrate_camera(d["obj"], d["img"], SIZE, **dict(kw, **over))


def distortion_map_px(K, dist, size=SIZE, grid=(25, 15)):
    """the model's pixel displacement on a grid over the frame: distorted pixel minus ideal pixel of the normalised points of
    the grid under K -> [gy, gx, 2].  What a rational model determines when its coefficients are not."""
    import lens_restated as lr
    u, v = np.meshgrid(np.linspace(0, size[0] - 1, grid[0]), np.linspace(0, size[1] - 1, grid[1]))
    x, y = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    xd, yd = lr.distort_normalized(x, y, np.asarray(dist)[:12])
    return np.stack([K[0, 0] * (xd - x), K[1, 1] * (yd - y)], -1)
