"""The inputs of the association and tracking tests (test_assign_cpu.py, test_assign_gpu.py) and of the generator of
tests/golden/assign.npz (tools/make_goldens.py: gen_assign): assignment problems of every kind, mask sets for
associate_det_trk, and box clips for the tracker.  Everything is seeded; NumPy only."""
import numpy as np

# one, two and three columns a lane, the lane-count edges, and both orientations of the transpose
SIZES = [(1, 1), (1, 5), (5, 1), (3, 3), (8, 13), (13, 8), (63, 64), (64, 65), (65, 130), (130, 65), (17, 200)]
KINDS = ("integer", "iou", "equal")
BIG = (1000, 1024)


def integer_costs(n, m, seed):
    """kind (a): integer-valued float64 drawn from [0, 2^30): every sum of at most 2^22 of them is exact"""
    return np.random.default_rng(seed).integers(0, 2 ** 30, size=(n, m)).astype(np.float64)


def iou_costs(n, m, seed):
    """kind (b): 1 - iou in float32 for an IoU-like matrix with about 60 % exact zeros: many equal costs of exactly 1"""
    rng = np.random.default_rng(seed)
    iou = (rng.random((n, m)) * (rng.random((n, m)) >= 0.6)).astype(np.float32)
    return np.float32(1) - iou


def equal_costs(n, m, seed=0):
    """kind (c): every assignment is optimal"""
    return np.full((n, m), 0.25, dtype=np.float64)


def costs(kind, n, m, seed):
    return {"integer": integer_costs, "iou": iou_costs, "equal": equal_costs}[kind](n, m, seed)


def seed_of(kind, n, m):
    return 1000 * KINDS.index(kind) + 7 * n + m


def nonfinite_costs():
    """kind (d): one NaN, one +inf, and a clean matrix between them (a batch: the clean one must not be disturbed)"""
    c = np.stack([integer_costs(6, 9, 41), integer_costs(6, 9, 42), integer_costs(6, 9, 43)])
    c[0, 4, 7] = np.nan
    c[2, 0, 0] = np.inf
    return c


def ragged_batch(seed=5):
    """kind (e): cost [B, N, M] with blocks n_rows x n_cols below N x M, zeros included; what lies outside a block is NaN,
    which must not be read as part of the problem"""
    N, M = 9, 70
    n_rows = np.array([9, 0, 3, 9, 5, 1, 0, 7], dtype=np.int32)
    n_cols = np.array([70, 4, 0, 5, 66, 1, 0, 64], dtype=np.int32)
    rng = np.random.default_rng(seed)
    c = np.full((len(n_rows), N, M), np.nan)
    for b, (r, k) in enumerate(zip(n_rows, n_cols)):
        c[b, :r, :k] = rng.integers(0, 2 ** 30, size=(r, k))
    return c, n_rows, n_cols


def unique_optimum(cost):
    """scipy's optimum is the only one: forbidding any one of its pairs (a cost of 1e18) strictly raises the total"""
    from scipy.optimize import linear_sum_assignment

    c = np.asarray(cost, dtype=np.float64)
    rows, cols = linear_sum_assignment(c)
    best = c[rows, cols].sum()
    for r, k in zip(rows, cols):
        d = c.copy()
        d[r, k] = 1e18
        rr, kk = linear_sum_assignment(d)
        if not d[rr, kk].sum() > best:
            return False
    return True


# ---- mask sets for associate_det_trk ---------------------------------------------------------------------------------------------
# name -> (N, M, H, W, shared core, seed).  With a core every mask holds a common rectangle plus a rectangle of its own: every
# IoU is positive; the seeds are chosen so that they are also distinct and the optimum unique (the CPU test asserts it).
ASSOC_CASES = {
    "core_3x4": (3, 4, 40, 56, True, 2),
    "core_5x5": (5, 5, 40, 56, True, 1),
    "core_6x3": (6, 3, 40, 56, True, 1),
    "core_odd": (4, 5, 37, 29, True, 2),       # 37 x 29: the pixel count is no multiple of 64
    "sparse_4x6": (4, 6, 40, 56, False, 5),
    "sparse_7x3": (7, 3, 40, 56, False, 6),
}
UNIQUE_CASES = [k for k in ASSOC_CASES if k.startswith("core")]
ASSOC_THRESHOLDS = dict(iou_threshold=0.35, iou_threshold_trk=0.45, new_det_thresh=0.5)


def _rect_masks(rng, n, H, W, core):
    m = np.zeros((n, H, W), dtype=np.uint8)
    for k in range(n):
        h, w = rng.integers(H // 5, H // 2), rng.integers(W // 5, W // 2)
        y, x = rng.integers(0, H - h), rng.integers(0, W - w)
        m[k, y:y + h, x:x + w] = 1
        if core:
            m[k, H // 3:H // 3 + H // 4, W // 3:W // 3 + W // 4] = 1
    return m


def assoc_case(name):
    """-> det_masks uint8 [N, H, W], track_masks uint8 [M, H, W], det_scores float32 [N]"""
    N, M, H, W, core, seed = ASSOC_CASES[name]
    rng = np.random.default_rng(seed)
    det, trk = _rect_masks(rng, N, H, W, core), _rect_masks(rng, M, H, W, core)
    if not core:
        trk[0] = 0                              # an empty track mask
        trk[-1] = det[0]                        # and one that is a detection exactly
    return det, trk, rng.random(N).astype(np.float32)


def assoc_clip(H=40, W=56, seed=9):
    """A clip of 5 frames with ragged counts -> det [5, 6, H, W], trk [5, 5, H, W], scores [5, 6], n_det, n_trk int32 [5]"""
    rng = np.random.default_rng(seed)
    n_det = np.array([6, 2, 0, 4, 5], dtype=np.int32)
    n_trk = np.array([5, 5, 3, 0, 2], dtype=np.int32)
    det = np.stack([_rect_masks(rng, 6, H, W, t % 2 == 0) for t in range(5)])
    trk = np.stack([_rect_masks(rng, 5, H, W, t % 2 == 0) for t in range(5)])
    return det, trk, rng.random((5, 6)).astype(np.float32), n_det, n_trk


# ---- box clips for the tracker ---------------------------------------------------------------------------------------------------
NAN_BOX = [np.nan] * 4


def _box(cx, cy, w=40.0, h=80.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def link_clips():
    """name -> (boxes float64 [T, N, 4], scores [T, N] or None, parameters, expected ids [T, N], expected (n_tracks, overflow))"""
    out = {}
    # two skiers cross: A moves right, B moves left half a box below, 6 pixels a frame, and they swap detection slots half way.
    # A frame's step leaves IoU 0.74 with one's own last box; the other's is at most 1/3 (half a box apart where they pass).
    T = 12
    b = np.zeros((T, 2, 4))
    want = np.zeros((T, 2), dtype=np.int32)
    for t in range(T):
        A, B = _box(100 + 6 * t, 200), _box(166 - 6 * t, 240)
        first = t < 6
        b[t] = [A, B] if first else [B, A]
        want[t] = [0, 1] if first else [1, 0]
    out["cross"] = (b, None, dict(iou_threshold=0.3, max_age=3, max_tracks=4), want, (2, 0))
    # a detection missing for max_age frames returns to its id; for max_age + 1 frames it is a new track
    for gap, name in ((3, "gap_max_age"), (4, "gap_longer")):
        T = 2 + gap + 2
        b = np.full((T, 1, 4), np.nan)
        want = np.full((T, 1), -1, dtype=np.int32)
        for t in list(range(2)) + list(range(2 + gap, T)):
            b[t, 0] = _box(50 + t, 60)
            want[t, 0] = 0 if t < 2 or gap == 3 else 1
        out[name] = (b, None, dict(iou_threshold=0.3, max_age=3, max_tracks=4), want, (1 if gap == 3 else 2, 0))
    # a frame without detections between frames with two
    b = np.array([[_box(50, 60), _box(200, 60)], [NAN_BOX, NAN_BOX], [_box(52, 60), _box(203, 61)]])
    out["empty_frame"] = (b, None, dict(iou_threshold=0.3, max_age=2, max_tracks=4), np.array([[0, 1], [-1, -1], [0, 1]], dtype=np.int32), (2, 0))
    # more detections than tracks: K = 2
    b = np.array([[_box(50, 60), _box(200, 60), _box(350, 60)], [_box(350, 61), _box(51, 60), _box(500, 60)]])
    out["overflow"] = (b, None, dict(iou_threshold=0.3, max_age=2, max_tracks=2),
                       np.array([[0, 1, -1], [-1, 0, -1]], dtype=np.int32), (2, 3))
    # a NaN coordinate makes a box no detection; a low score keeps a detection from starting a track, not from matching one
    b = np.array([[_box(50, 60), [10.0, 10.0, np.nan, 50.0], _box(300, 60)], [_box(51, 60), _box(200, 60), _box(301, 60)],
                  [_box(52, 60), _box(201, 60), _box(302, 60)]])
    s = np.array([[0.9, 0.9, 0.2], [0.1, 0.9, 0.9], [0.9, 0.1, 0.1]])
    out["nan_and_scores"] = (b, s, dict(iou_threshold=0.3, max_age=2, new_score=0.5, max_tracks=4),
                             np.array([[0, -1, -1], [0, 1, 2], [0, 1, 2]], dtype=np.int32), (3, 0))
    return out


def random_clips(B=3, T=40, N=7, seed=11):
    """Seeded random walks with drop-outs and swapped slots -> boxes [B, T, N, 4], scores [B, T, N]"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(100, 900, size=(B, 1, N, 2)) + np.cumsum(rng.normal(0, 14, size=(B, T, N, 2)), axis=1)
    size = rng.uniform(30, 90, size=(B, 1, N, 2))
    boxes = np.concatenate([centre - size / 2, centre + size / 2], axis=-1)
    boxes[rng.random((B, T, N)) < 0.3] = np.nan
    for b in range(B):
        for t in range(T):
            boxes[b, t] = boxes[b, t, rng.permutation(N)]
    return boxes, rng.random((B, T, N))
