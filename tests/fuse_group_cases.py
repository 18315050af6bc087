"""Seeded inputs of tests/test_fuse_group_cpu.py and tests/test_fuse_group_gpu.py (and of tools/make_goldens.py's
"fuse_group" generator, which runs the reference on the three *_golden_* inputs), and the host side of the comparison:
the functions of skiing_analysis_pytorch_amd/fuse.py and skeleton.py, pinned to the reference by
tests/golden/fuse_group.npz.  Every host result is computed once per process and shared."""
import functools
import itertools
from pathlib import Path

import numpy as np

from skiing_analysis_pytorch_amd import fuse, skeleton

from fuse_cases import _project, _rot_y, _walk, close  # noqa: F401  (close is re-exported)

NAN = np.nan
GOLDEN = Path(__file__).resolve().parent / "golden" / "fuse_group.npz"
IDS15 = skeleton.MHR70_15_IDS
KEYS15 = dict(root_idx=14, left_hip_idx=11, right_hip_idx=12, left_shoulder_idx=5, right_shoulder_idx=6)   # fuse/main_unity.py
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def id_of(pos):
    """the MHR-70 id at a position of the 15-joint array; a position outside it becomes an id that is not a target"""
    return IDS15[pos] if 0 <= pos < 15 else 1000 + pos


def _body(rng, J):
    return rng.uniform(-0.5, 0.5, size=(J, 3)) * np.array([0.6, 1.8, 0.4])


# ---- joint quality ----------------------------------------------------------------------------------------------------
Q_NEVER, Q_LONE = 12, 0            # of the golden clip: a joint that is never seen, a joint without an edge


@functools.lru_cache(maxsize=None)
def quality_golden_case():
    """the clip the reference's no-GT quality is recorded on: T = 9, the 15 MHR-70 joints, BONE_EDGES plus a repeated edge, a
    self-edge and two edges with an endpoint that is no target joint"""
    rng = np.random.default_rng(21)
    T, J, W, H = 9, 15, 640, 360
    X = _walk(rng, _body(rng, J), T, amp=0.05)
    X[:, Q_NEVER] = NAN                # Hand_R: its edge has no sample, its neighbour loses an edge
    X[3, 4] = NAN                      # lowerarm_l missing in one frame: 8 samples (even) for its two edges
    X[5, 14, 1] = NAN                  # the neck with one coordinate missing
    X[6, 2] = NAN                      # a gap: q_temp restarts at frame 7
    U = np.stack([rng.uniform(1, W - 1, size=(T, J)), rng.uniform(1, H - 1, size=(T, J))], axis=-1)
    U[0, 0, 0] = 0.0                   # u exactly 0: inside
    U[1, 1, 0] = float(W)              # u exactly width: outside
    U[2, 2, 1] = -3.0                  # negative v
    U[3, 3, 0] = NAN
    U[4, 4, 1] = np.inf
    U[5, 5, 1] = float(H)
    U[:, 7] = NAN                      # absent from the reference's dict
    edges = list(skeleton.MHR70_15_EDGES) + [(2, 4), (6, 6), (3, 20), (17, 2)]
    return dict(X=X, U=U, u_absent=(7,), width=W, height=H, edges=edges, beta_temp=1.5, w_bone=1.0, w_temp=0.3, w_san=0.2)


QUALITY_T = (0, 1, 2, 5, 6, 67, 130)
QUALITY_J = (15, 17, 64, 65, 128)
QUALITY_SIZE = (640.0, 360.0)
QUALITY_KW = dict(beta_temp=1.25, w_bone=0.9, w_temp=0.3, w_san=0.2)


@functools.lru_cache(maxsize=None)
def quality_case(T, J, V=1):
    """X [V, T, J, 3], U [V, T, J, 2], edges: a chain 0-1-..-(J-2) with every third link doubled back, a repeated edge, a
    self-edge, an out-of-range edge; joint J - 1 has no edge, joint 3 is never seen (its edges have no sample), a tenth of the
    rows are missing, 2D points sit on and beyond the borders"""
    rng = np.random.default_rng(1000 * T + 10 * J + V)
    X = np.stack([_walk(rng, _body(rng, J), T, amp=0.06) for _ in range(V)]) if T else np.zeros((V, 0, J, 3))
    X = X + 0.003 * rng.normal(size=X.shape)
    X[rng.random(size=X.shape[:3]) < 0.1] = NAN
    X[:, :, 3] = NAN
    if T > 1:
        X[:, 1, 5, 2] = NAN
    W, H = QUALITY_SIZE
    U = np.stack([rng.uniform(-20, W + 20, size=X.shape[:3]), rng.uniform(-20, H + 20, size=X.shape[:3])], axis=-1)
    if T:
        U[:, 0, 0] = (0.0, 10.0)
        U[:, 0, 1] = (W, 10.0)
        U[:, 0, 2] = (10.0, -1.0)
        U[:, 0, 4] = (NAN, 10.0)
        U[:, 0, 6] = (10.0, np.inf)
        U[:, 0, 7] = (10.0, H)
        U[:, 0, 8] = (W - 0.5, 0.0)
    edges = [(j, j + 1) for j in range(J - 2)] + [(j + 2, j) for j in range(0, J - 4, 3)]
    edges += [(1, 2), (6, 6), (2, J), (-1, 4), (J + 5, J + 6)]
    return dict(X=X, U=U, edges=edges)


def host_quality(X, U, edges, size=QUALITY_SIZE, med_lens=None, bias=None, **kw):
    """fuse.compute_q_nogt per view -> dict of [V, T, J] arrays and med_lens [V, E]"""
    V = X.shape[0]
    size = np.broadcast_to(np.asarray(size, dtype=np.float64), (V, 2))
    per = []
    for v in range(V):
        b = None if bias is None else (bias if np.ndim(bias) == 1 else bias[v])
        per.append(fuse.compute_q_nogt(X[v], None if U is None else U[v], edges=edges, width=size[v, 0], height=size[v, 1],
                                       med_lens=None if med_lens is None else med_lens[v], bias=b, **kw))
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


@functools.lru_cache(maxsize=None)
def host_quality_case(T, J, V=1, with_U=True):
    c = quality_case(T, J, V)
    return host_quality(c["X"], c["U"] if with_U else None, c["edges"], **QUALITY_KW)


# ---- group fusion -----------------------------------------------------------------------------------------------------
def _group_views(rng, V, T, J, body=None):
    body = _body(rng, J) if body is None else body
    X0 = _walk(rng, body, T, amp=0.04)
    X0 -= X0[:, :1].mean(axis=0, keepdims=True)
    X = np.stack([X0] + [(1.0 + 0.02 * v) * (X0 @ _rot_y(0.5 * v).T) + np.array([0.1 * v, 0.05, 0.2 * v]) + 0.02 * rng.normal(size=X0.shape)
                         for v in range(1, V)])
    return X, np.stack([_project(rng, X[v]) for v in range(V)])


@functools.lru_cache(maxsize=None)
def group_golden_case():
    """three views of the 15 MHR-70 joints, T = 6, every view with at least 8 fit points in every frame (the reference raises
    below that)"""
    rng = np.random.default_rng(31)
    X, U = _group_views(rng, 3, 6, 15)
    X[0, 1, 3] = NAN
    X[1, 2, [3, 7]] = NAN
    U[2, 3, 4] = NAN
    X[1, 4, 11] = NAN                  # a key joint of view 1: its cross-view confidences are 0
    X[0, 5, 9] = NAN                   # missing in two views of three
    X[2, 5, 9] = NAN
    X[0, :2, 8] = NAN                  # not seen by two views at the start: NaN in their smoothed file too
    X[2, :2, 8] = NAN
    return dict(X=X, U=U, sigma_px=12.0, sigma_3d=0.08,
                ema=dict(alpha=0.7, adaptive=True, alpha_min=0.45, alpha_max=0.92, speed_gain=0.25))


@functools.lru_cache(maxsize=None)
def group_case(V):
    """[V, 5, 70, 3] views with the special frames of fuse_cases' two-view clip: NaN 3D and 2D joints on both lane halves,
    fewer than 3 common joints, fewer than min_points fit rows, a missing key joint"""
    from fuse_cases import KEYS70
    rng = np.random.default_rng(40 + V)
    X, U = _group_views(rng, V, 5, 70)
    X[0, 1, [3, 17, 64, 69]] = NAN
    X[V - 1, 1, [17, 30, 65]] = NAN
    U[0, 2, [2, 40, 68]] = NAN
    U[V - 1, 2, 41, 0] = NAN
    X[0, 3, 2:] = NAN                  # 2 joints in common with every other view; 2 fit rows
    U[V - 1, 4, 7:] = NAN              # 7 fit rows
    X[V - 1, 0, 10] = NAN              # a key joint
    return dict(X=X, U=U, kw=dict(**KEYS70, sigma_px=12.0, sigma_3d=0.08, scale_mode="hip", min_points=8))


def pairs_of(V):
    return list(itertools.combinations(range(V), 2))


def host_view_conf(X, U, kw):
    """per view and frame fuse.weakpersp_reproj_confidence -> conf, err [V, T, J], fit_ok [V, T]; where the host raises conf is
    0, err NaN and fit_ok False, the rule of the device build"""
    V, T, J = X.shape[:3]
    conf, err, ok = np.zeros((V, T, J)), np.full((V, T, J), NAN), np.zeros((V, T), dtype=bool)
    for v in range(V):
        for t in range(T):
            try:
                conf[v, t], err[v, t], _, _ = fuse.weakpersp_reproj_confidence(X[v, t], U[v, t], sigma_px=kw["sigma_px"],
                                                                               min_points=kw.get("min_points", 8))
                ok[v, t] = True
            except ValueError:
                pass
    return conf, err, ok


def host_group(X, U, kw, align=False, quality=None):
    """fuse/main_unity.py's _fuse_pair (align=False) or fuse/main_raw.py's frame body (align=True) with fuse.py's functions for
    every pair -> dict of arrays as geometry.fuse_group returns them"""
    V, T, J = X.shape[:3]
    pairs = pairs_of(V)
    P = len(pairs)
    out = {k: np.full((P, T, J, 3), NAN) for k in ("fused", "aligned")}
    out |= {k: np.full((P, T, J), NAN) for k in ("q_a", "q_b", "conf_x", "dist")}
    out["pairs"] = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    if quality is None:
        out["conf"], out["err"], out["fit_ok"] = conf, _, _ = host_view_conf(X, U, kw)
    keys = {k: v for k, v in kw.items() if k.endswith("_idx")}
    for p, (a, b) in enumerate(pairs):
        for t in range(T):
            al = fuse.align_right_to_left(X[a, t], X[b, t]) if align else X[b, t].copy()
            if quality is None:
                cx, d, _, _, _ = fuse.crossview_consistency_confidence(X[a, t], X[b, t], **keys, sigma_3d=kw["sigma_3d"],
                                                                       scale_mode=kw.get("scale_mode", "hip"))
                qa, qb = np.sqrt(conf[a, t] * cx), np.sqrt(conf[b, t] * cx)
                out["conf_x"][p, t], out["dist"][p, t] = cx, d
            else:
                qa, qb = quality[a, t], quality[b, t]
            out["aligned"][p, t], out["q_a"][p, t], out["q_b"][p, t] = al, qa, qb
            out["fused"][p, t] = fuse.fuse_frame_3d(X[a, t], al, qa, qb)
    return out


# ---- skeleton conversion ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def skeleton_golden_inputs():
    """name -> array; names starting with "coco" go through coco_to_h36m, the others through h36m_to_coco"""
    rng = np.random.default_rng(51)
    coco3 = rng.normal(size=(5, 17, 3))
    coco3[1, 1] = NAN                  # an eye: the head
    coco3[2, 11, 0] = NAN              # one coordinate of a hip: pelvis and spine in x
    coco3[3, 0] = NAN                  # the nose: neck and head
    coco2 = rng.normal(size=(5, 17, 2))
    coco2[4, 6] = NAN
    h36m3 = rng.normal(size=(4, 17, 3))
    h36m3_nan = h36m3.copy()
    h36m3_nan[1, 10] = NAN             # the head: eyes and ears of the frame
    h36m3_nan[3, 11, 2] = NAN          # a shoulder coordinate: the clip mean is NaN, which takes the normal branch
    h36m2 = rng.normal(size=(4, 17, 2))
    deg3, deg2 = h36m3.copy(), h36m2.copy()
    deg3[:, 11] = deg3[:, 14]          # coincident shoulders in every frame: the degenerate branch
    deg2[:, 11] = deg2[:, 14]
    return {"coco3": coco3, "coco2": coco2, "coco3_single": coco3[0].copy(), "coco2_single": coco2[1].copy(),
            "h36m3": h36m3, "h36m3_nan": h36m3_nan, "h36m2": h36m2, "h36m3_single": h36m3[2].copy(), "h36m2_single": h36m2[0].copy(),
            "h36m3_deg": deg3, "h36m2_deg": deg2}


def host_skeleton(name, variant):
    """the host conversion of a golden input; variant: "h36m", "h36m_nohead", "coco", "coco_face" """
    X = skeleton_golden_inputs()[name]
    if variant.startswith("h36m"):
        return skeleton.coco_to_h36m(X, synthesize_head=variant == "h36m")
    return skeleton.h36m_to_coco(X, synthesize_face=variant == "coco_face")


def skeleton_variants(name):
    return ("h36m", "h36m_nohead") if name.startswith("coco") else ("coco", "coco_face")


def write_camera_npz(path, p2d, p3d, key="outputs"):
    """a file in the reference's layout: per-frame records of 70 joints, the 15 target rows filled"""
    frames = []
    for t in range(p3d.shape[0]):
        k2, k3 = np.full((70, 2), 1e6), np.full((70, 3), 1e6)
        k2[IDS15], k3[IDS15] = p2d[t], p3d[t]
        frames.append({"pred_keypoints_2d": k2.astype(np.float64), "pred_keypoints_3d": k3, "bbox": np.zeros(4)})
    np.savez(path, **{key: np.array(frames, dtype=object)})


def bits_equal(a, b):
    """two float arrays are the same bits (NaN payloads aside: NaN matches NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))
