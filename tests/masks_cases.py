"""The named inputs of the mask analysis tests (tests/test_masks_cpu.py, tests/test_masks_gpu.py, tools/make_goldens.py's
gen_masks).  Shapes: neither side of SIZES divides a 64 x 16 tile, H W is no multiple of 64 (the last packed word is partial)
and the rows are not dword-aligned; DEGENERATE holds the one-pixel, one-row and one-column images."""
import numpy as np

SIZES = ((37, 70), (67, 131))
DEGENERATE = ((1, 1), (1, 70), (37, 1))
B = 3
DENSITIES = (0.41, 0.5, 0.6, 0.9)
MANY_MAX_COMPONENTS = 8
NMS_COUNTS = (1, 2, 63, 64, 65, 200)
NMS_THRESHOLDS = (0.0, 0.5, 1.0)
IOU_SHAPES = ((5, 3), (1, 1), (0, 3), (17, 17))


def batch(m):
    """a mask -> B = 3 masks: itself, mirrored left-right, mirrored top-bottom"""
    return np.ascontiguousarray(np.stack([m, m[:, ::-1], m[::-1, :]]))


def rings(H, W):
    """two nested rectangular rings with a dot in the middle"""
    m = np.zeros((H, W), dtype=np.uint8)
    for k in (1, 4):
        m[k:H - k, k:W - k] = 1
        m[k + 1:H - k - 1, k + 1:W - k - 1] = 0
    m[H // 2, W // 2] = 1
    return m


def component_cases(H, W):
    """name -> mask uint8 [H, W]"""
    rng = np.random.default_rng(H * 1000 + W)
    ys, xs = np.mgrid[0:H, 0:W]
    c = {"empty": np.zeros((H, W), dtype=np.uint8), "full": np.ones((H, W), dtype=np.uint8)}
    corners = np.zeros((H, W), dtype=np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 1
    c["corners"] = corners
    c["checkerboard"] = ((ys + xs) % 2 == 0).astype(np.uint8)
    c["diagonal"] = (xs == np.minimum(ys, W - 1)).astype(np.uint8)
    # every even row, joined to the next at the right end after rows 0, 4, .. and at the left end after rows 2, 6, ..
    c["serpentine"] = ((ys % 2 == 0) | ((ys % 4 == 1) & (xs == W - 1)) | ((ys % 4 == 3) & (xs == 0))).astype(np.uint8)
    c["comb"] = ((ys == 0) | (xs % 2 == 0)).astype(np.uint8)
    if H >= 12 and W >= 12:
        c["rings"] = rings(H, W)
    # two arms that meet only in the last row
    c["u"] = (((xs == 1) | (xs == W - 2) | (ys == H - 1)) & (xs >= 1) & (xs <= W - 2)).astype(np.uint8)
    for d in DENSITIES:
        c[f"random_{d}"] = (rng.random((H, W)) < d).astype(np.uint8)
    c["many"] = ((ys % 3 == 0) & (xs % 3 == 0)).astype(np.uint8)   # isolated dots: far more than MANY_MAX_COMPONENTS
    return c


def edt_cases(H, W):
    """name -> (mask uint8 [H, W], border_zero)"""
    rng = np.random.default_rng(H * 77 + W)
    ys, xs = np.mgrid[0:H, 0:W]
    c = {}
    m = np.ones((H, W), dtype=np.uint8)
    m[0, 0] = 0
    c["zero_in_corner"] = (m, False)
    m = np.ones((H, W), dtype=np.uint8)
    m[H // 2, W // 2] = 0
    c["zero_in_centre"] = (m, False)
    c["zero_in_centre_border"] = (m, True)
    c["no_zero"] = (np.ones((H, W), dtype=np.uint8), False)
    c["no_zero_border"] = (np.ones((H, W), dtype=np.uint8), True)
    c["all_zero"] = (np.zeros((H, W), dtype=np.uint8), False)
    c["all_zero_border"] = (np.zeros((H, W), dtype=np.uint8), True)
    c["stripes_vertical"] = ((xs % 9 != 0).astype(np.uint8), False)
    c["stripes_horizontal"] = ((ys % 7 != 3).astype(np.uint8), True)
    for share in (0.01, 0.1, 0.5):
        z = (rng.random((H, W)) >= share).astype(np.uint8)
        c[f"random_{share}"] = (z, False)
        c[f"random_{share}_border"] = (z, True)
    return c


def two_maxima(H, W):
    """two equal squares: the inner point's largest d2 is met twice (and more: the first in raster order wins)"""
    m = np.zeros((H, W), dtype=np.uint8)
    m[10:17, 40:47] = 1
    m[20:27, 5:12] = 1
    return m


def iou_masks(n, H, W, seed):
    """[n, H, W] uint8: random blobs, then an identical pair, a disjoint pair and empty masks where n allows"""
    rng = np.random.default_rng(seed)
    m = (rng.random((n, H, W)) < rng.uniform(0.1, 0.7, (n, 1, 1))).astype(np.uint8)
    if n >= 5:
        m[1] = m[0]
        m[2] = 0
        m[3] = 1 - m[0]
        m[4] = 0
        m[4, H - 1, W - 1] = 1    # the last pixel: the partial word's last bit
    return m


def nms_problem(n, seed, ties=False, nan=False, holes=False):
    """-> iou float32 [n, n] (symmetric, ones on the diagonal), scores float32 [n], valid bool [n] or None"""
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)).astype(np.float32)
    io = np.maximum(a, a.T)
    io[rng.random((n, n)) < 0.3] = 0.0
    io = np.minimum(io, io.T)
    io[rng.random((n, n)) < 0.05] = 1.0
    io = np.maximum(io, io.T)
    np.fill_diagonal(io, 1.0)
    scores = rng.random(n).astype(np.float32)
    if ties:
        scores = (np.round(scores * 4) / 4).astype(np.float32)
        scores[::7] = np.float32(-0.0)    # ties with the +0 the rounding leaves
    if nan and n > 1:
        scores[n // 2] = np.nan
    valid = (rng.random(n) < 0.7) if holes else None
    return io, scores, valid


def nms_chain():
    """a suppresses b, b would suppress c, a does not: c must be kept"""
    io = np.array([[1.0, 0.8, 0.1], [0.8, 1.0, 0.8], [0.1, 0.8, 1.0]], dtype=np.float32)
    return io, np.array([0.9, 0.8, 0.7], dtype=np.float32)


def person_clip(T, N, H, W):
    """[T, N, H, W] uint8: a moving rectangle with a hole and a sprinkle; the last mask of the last frame is empty"""
    m = np.zeros((T, N, H, W), dtype=np.uint8)
    for t in range(T):
        for n in range(N):
            x0, y0 = 5 + 7 * t + 20 * n, 4 + 3 * t
            m[t, n, y0:y0 + 18, x0:x0 + 11] = 1
            m[t, n, y0 + 5, x0 + 4] = 0       # a hole
            m[t, n, H - 2, 1 + n] = 1         # a sprinkle
    m[-1, -1] = 0
    return m
