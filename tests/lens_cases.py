"""The cases of the lens tests (tests/test_lens_cpu.py, tests/test_lens_gpu.py) and of tools/make_goldens.py gen_lens:
inputs only, built from fixed seeds; nothing here knows a result."""
from pathlib import Path

import numpy as np

import lens_restated as lr

GOLDEN = Path(__file__).resolve().parent / "golden"

# ---- the reference's cv2-free model (vggt/vggt/dependency/distortion.py): 1, 2 and 4 parameters ----------------------------
REF_P4 = np.array([[0.177, -0.457, -0.0027, -0.0033], [-0.21, 0.06, 0.0011, -0.0007]])
REF_P2 = REF_P4[:, :2].copy()
REF_P1 = REF_P4[:, :1].copy()
REF_INVERTIBLE_R2 = 0.46     # the first row of REF_P4 is one-to-one up to about here and folds over beyond r2 ~ 0.6
FOLD_POINT_NORMALIZED = (0.9, 0.6)   # a distorted position no point maps to under REF_P4[0] (|x_d| never exceeds ~0.77)


def ref_forward_points():
    """normalised (u, v) [2, 200] for the forward comparison, |u|, |v| <= 0.8"""
    rng = np.random.default_rng(20)
    return rng.uniform(-0.8, 0.8, (2, 200)), rng.uniform(-0.8, 0.8, (2, 200))


def ref_inverse_truth():
    """undistorted normalised points [1, 300, 2] inside the invertible range of REF_P4[0] (r2 <= 0.45), the disc's rim and
    centre included"""
    rng = np.random.default_rng(21)
    r = np.sqrt(rng.uniform(0, 0.45, 300))
    r[:8] = np.sqrt(0.45)
    r[8] = 0.0
    a = rng.uniform(0, 2 * np.pi, 300)
    return np.stack([r * np.cos(a), r * np.sin(a)], -1)[None]


# ---- calibrations --------------------------------------------------------------------------------------------------------
def fixture_calibration():
    """(K [3, 3], dist [14], (w, h)) of tests/golden/calibration.npz"""
    with np.load(GOLDEN / "calibration.npz", allow_pickle=False) as z:
        return z["camera_matrix"].astype(np.float64), z["dist_coeffs"].reshape(-1).astype(np.float64), tuple(int(v) for v in z["image_size"])


def full_frame_grid(w=1920, h=1080, nx=49, ny=28):
    """pixel grid [ny * nx, 2] over the whole frame, the four corners included"""
    u, v = np.meshgrid(np.linspace(0, w - 1, nx), np.linspace(0, h - 1, ny))
    return np.stack([u.ravel(), v.ravel()], -1)


# one coefficient vector of every length OpenCV hands out; moderate values, invertible over a frame with fx ~ width
COEFFS = {
    4: [-0.28, 0.09, 0.0012, -0.0008],
    5: [-0.28, 0.09, 0.0012, -0.0008, -0.011],
    8: [-0.31, 0.12, -0.0009, 0.0015, 0.02, 0.05, -0.03, 0.004],
    12: [-0.25, 0.07, 0.0007, 0.0011, -0.006, 0.03, 0.01, -0.002, 0.0013, -0.0004, -0.0009, 0.0006],
    14: [-0.25, 0.07, 0.0007, 0.0011, -0.006, 0.03, 0.01, -0.002, 0.0013, -0.0004, -0.0009, 0.0006, 0.0, 0.0],
}
OTHER = [0.11, -0.04, -0.002, 0.0017, 0.008, -0.02, 0.006, 0.0, -0.0011, 0.0002, 0.0005, -0.0003]   # the second camera
POINT_COUNTS = (1, 63, 65, 17 * 243)


def small_K(w, h, f=0.9, dx=0.37, dy=-0.21):
    """a plausible K for a w x h frame whose entries are no round binary fractions"""
    return np.array([[f * w + 0.123, 0.0, (w - 1) / 2 + dx], [0.0, f * w * 1.003 + 0.0457, (h - 1) / 2 + dy], [0.0, 0.0, 1.0]])


def point_case(k, n, seed=0, w=640, h=360):
    """two cameras with different K and coefficients, n distorted pixels each over (and a little beyond) the frame:
    -> x [2, n, 2], K [2, 3, 3], dist [2, k], P [2, 3, 3]"""
    rng = np.random.default_rng(1000 * k + n + seed)
    K = np.stack([small_K(w, h), small_K(w, h, 0.8, -1.3, 0.9)])
    other = np.zeros(max(k, 12))
    other[:12] = OTHER
    dist = np.stack([np.asarray(COEFFS[k], np.float64), other[:k] if k != 14 else np.r_[other[:12], 0, 0]])
    x = rng.uniform([-10, -10], [w + 10, h + 10], (2, n, 2))
    P = np.stack([small_K(w, h, 0.7, 2.2, -1.1), small_K(w, h, 1.1, 0.3, 0.4)])
    return x, K, dist, P


# ---- frames ----------------------------------------------------------------------------------------------------------------
def image_cases():
    """name -> dict(H, W, ch, out_size (w, h) | None, K [2, 3, 3], dist [2, k], new_K [2, 3, 3] | None): C = 2 cameras, F = 3"""
    cases = {}
    K11 = np.array([[1.3, 0, 0.1], [0, 1.2, -0.2], [0, 0, 1.0]])
    cases["1x1"] = dict(H=1, W=1, ch=3, out_size=None, K=np.stack([K11, K11 * [[1.1], [0.9], [1]]]), dist=np.stack([COEFFS[4], OTHER[:4]]),
                        new_K=None)
    for name, H, W, ch, out_size in (("37x53", 37, 53, 3, (61, 29)), ("37x53_grey", 37, 53, 1, (50, 41)),
                                     ("64x256", 64, 256, 3, None), ("64x256_grey", 64, 256, 1, (260, 66))):
        K = np.stack([small_K(W, H), small_K(W, H, 0.8, -1.3, 0.9)])
        ow, oh = out_size or (W, H)
        new_K = np.stack([small_K(ow, oh, 0.75, 0.6, 0.2), small_K(ow, oh, 0.85, -0.4, 1.3)])
        cases[name] = dict(H=H, W=W, ch=ch, out_size=out_size, K=K, dist=np.stack([COEFFS[12], OTHER]), new_K=new_K)
    K, d, (w, h) = fixture_calibration()
    Ks = K.copy()
    Ks[0] *= 480 / w
    Ks[1] *= 270 / h
    cases["270x480_fixture"] = dict(H=270, W=480, ch=3, out_size=None, K=np.stack([Ks, Ks]), dist=np.stack([d, np.r_[OTHER, 0, 0]]),
                                    new_K=None)
    return cases


def images_of(case, C=2, F=3, seed=5):
    """uint8 [C, F, H, W, ch]: smooth structure plus noise, so that interpolation matters and values spread over 0..255"""
    H, W, ch = case["H"], case["W"], case["ch"]
    rng = np.random.default_rng(seed + 7 * H + W + ch)
    v, u = np.mgrid[0:H, 0:W]
    base = 127 + 90 * np.sin(u[None, None, ..., None] / 3.1 + rng.uniform(0, 6, (C, F, 1, 1, ch))) * np.cos(v[None, None, ..., None] / 4.3)
    return np.clip(base + rng.integers(-37, 38, (C, F, H, W, ch)), 0, 255).astype(np.uint8)


def restated_frames(case, imgs):
    """the restatement's (uint8 result, near-tie mask) for every camera and frame of a case"""
    C, F = imgs.shape[:2]
    out, tie = [], []
    for c in range(C):
        new_K = None if case["new_K"] is None else case["new_K"][c]
        vals = [lr.undistort_image_values(imgs[c, f], case["K"][c], case["dist"][c], new_K, case["out_size"]) for f in range(F)]
        out.append([np.floor(v + 0.5).astype(np.uint8) for v in vals])
        tie.append([lr.near_tie(v) for v in vals])
    return np.array(out), np.array(tie)


# ---- a distorted two-camera rig ---------------------------------------------------------------------------------------------
def rig_case():
    """Two cameras with the fixture's lens looking at 25 joints per step whose images cover camera 0's frame, corners included.
    K, R, t are float32-exact (the triangulation takes float32), the joints are the truth.
    -> dict(K [T, 2, 3, 3], R, t, X [T, J, 3], kp [T, 2, J, 2] distorted pixels, kp_ideal (no lens), dist [14])"""
    K0, d, (w, h) = fixture_calibration()
    K0 = K0.astype(np.float32).astype(np.float64)
    ang = np.deg2rad(-24.0)
    R1 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]).astype(np.float32).astype(np.float64)
    t1 = np.array([0.85, 0.02, 0.18], np.float32).astype(np.float64)
    R = np.stack([np.eye(3), R1])
    t = np.stack([np.zeros(3), t1])
    T = 2
    gu, gv = np.meshgrid(np.linspace(1.0, w - 2.0, 5), np.linspace(1.0, h - 2.0, 5))
    px0 = np.stack([gu.ravel(), gv.ravel()], -1)                       # distorted pixels in camera 0, the corners included
    rays, _ = lr.undistort_points(px0, K0, d, normalized=True)
    rng = np.random.default_rng(31)
    X = np.empty((T, 25, 3))
    for i in range(T):
        z = rng.uniform(1.9, 2.3, 25)
        X[i] = np.stack([rays[:, 0] * z, rays[:, 1] * z, z], -1)
    kp = np.stack([np.stack([lr.project_points(X[i], R[v], t[v], K0, d)[0] for v in range(2)]) for i in range(T)])
    kp_ideal = np.stack([np.stack([lr.project_points(X[i], R[v], t[v], K0, None)[0] for v in range(2)]) for i in range(T)])
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a, (T,) + a.shape))   # noqa: E731
    return dict(K=tile(np.stack([K0, K0])), R=tile(R), t=tile(t), X=X, kp=kp, kp_ideal=kp_ideal, dist=d)


def checkerboards(K, dist, cols=9, rows=6, boards=3):
    """the corners of `boards` tilted chessboards as the lens images them: list of [rows * cols, 2] distorted pixels"""
    rng = np.random.default_rng(41)
    gx, gy = np.meshgrid(np.arange(cols) - (cols - 1) / 2, np.arange(rows) - (rows - 1) / 2)
    obj = np.stack([gx.ravel() * 0.16, gy.ravel() * 0.16, np.zeros(rows * cols)], -1)
    out = []
    for _ in range(boards):
        ax, ay, az = rng.uniform(-0.35, 0.35, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
        out.append(lr.project_points(obj, Rz @ Ry @ Rx, np.array([rng.uniform(-0.25, 0.25), rng.uniform(-0.1, 0.1), 1.0]), K, dist)[0])
    return out
