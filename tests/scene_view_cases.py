"""Inputs of the scene-view tests (CPU and GPU): views, clouds with every kind of awkward row, and primitive lists."""
import numpy as np

import scene_view_restated as sr

SIZES = [(37, 53), (70, 130)]     # (H, W): no multiple of the 16 x 64 tile, rows not dword-aligned; the second spans several tiles
COUNTS = [0, 1, 64, 300]
N_POINTS = 5000
NEAR, FAR = 0.5, 6.0


def views(F, H, W, ortho=False):
    """F cameras on an arc around the origin, about 3 away, looking at it, world +z up"""
    out = []
    for f in range(F):
        a = 0.4 * f - 0.3
        eye = np.array([3.0 * np.cos(a), 3.0 * np.sin(a), 0.6 + 0.2 * f])
        fx = W / 2.4 if ortho else 0.9 * W
        out.append(sr.look_at(eye, [0.0, 0.0, 0.1 * f], [0.0, 0.0, 1.0], fx, fx, W / 2.0 + 0.25, H / 2.0 - 0.5, NEAR, FAR, ortho))
    return np.stack(out)


def cloud(P, N=N_POINTS, seed=0):
    """xyz f32 [P, N, 3], rgb u8 [P, N, 3]: a box wider than any view (points leave through all four edges), exact duplicates
    (the same pixel AND the same w: the tie rule decides), NaN and +-inf rows, rows behind the near plane and beyond the far"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.6, 1.6, size=(P, N, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(P, N, 3), dtype=np.uint8)
    if N >= 1000:
        xyz[:, 200:260] = xyz[:, 100:160]                     # duplicates, later index wins
        xyz[:, 300:330] = xyz[:, 100:130]
        xyz[:, 400, 0], xyz[:, 401, 1], xyz[:, 402, 2] = np.nan, np.inf, -np.inf
        xyz[:, 403] = np.nan
        xyz[:, 410:440] = rng.uniform(2.6, 2.9, size=(P, 30, 1)).astype(np.float32) * np.array([1.0, 0.0, 0.2], dtype=np.float32)   # at the eyes
        xyz[:, 440:470] = rng.uniform(-9.0, -5.0, size=(P, 30, 3)).astype(np.float32)                                                # too far
    return xyz, rgb


def prim(kind, x0, y0, x1, y1, r, colour, w0, w1):
    return [kind, x0, y0, x1, y1, r, colour, w0, w1, 0, 0, 0]


def random_prims(M, H, W, seed):
    """every kind, positions from outside the frame on all sides, radii from 0, depths over the whole range and beyond it"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((M, 12), dtype=np.int32)
    rec[:, 0] = rng.choice([0, 1, 2, 2, 2, 1, 7, -1], size=M)
    for c, hi in ((1, W), (2, H), (3, W), (4, H)):
        rec[:, c] = rng.integers(-20 * 16, (hi + 20) * 16, size=M)
    rec[:, 5] = rng.choice([0, 3, 8, 16, 24, 40, 90, -5], size=M)
    rec[:, 6] = rng.integers(0, 1 << 24, size=M)
    rec[:, 7] = rng.integers(-5, sr.W_ONE + 1000, size=M)
    rec[:, 8] = rng.integers(1, sr.W_ONE, size=M)
    rec[:, 9:] = rng.integers(-9, 9, size=(M, 3))              # the reserved words are not read
    return rec


def counted(M, H, W):
    return random_prims(M, H, W, seed=100 + M)


def one_tile(M):
    """M primitives that all sit on the first 64 x 16 tile"""
    rng = np.random.default_rng(7)
    rec = np.zeros((M, 12), dtype=np.int32)
    rec[:, 0] = rng.choice([1, 2], size=M)
    rec[:, 1], rec[:, 3] = rng.integers(0, 36 * 16, size=M), rng.integers(0, 36 * 16, size=M)
    rec[:, 2], rec[:, 4] = rng.integers(0, 15 * 16, size=M), rng.integers(0, 15 * 16, size=M)
    rec[:, 5] = rng.integers(0, 30, size=M)
    rec[:, 6] = rng.integers(0, 1 << 24, size=M)
    rec[:, 7], rec[:, 8] = rng.integers(1, sr.W_ONE, size=M), rng.integers(1, sr.W_ONE, size=M)
    return rec


def special_prims(H, W):
    """degenerate capsules, none records, unknown kinds, radius 0, negative and larger than the frame, saturating positions,
    two crossing capsules of different depth slopes, equal-w primitive over primitive"""
    big = 16 * 4 * max(H, W)
    return np.array([
        prim(1, 16 * (W // 2), 16 * (H // 2), 0, 0, big, 0x101010, 5, 5),                      # larger than the frame, far away
        prim(2, 16 * 5, 16 * 5, 16 * 5, 16 * 5, 40, 0x0000FF, 1000, 9),                        # a = b: the disc, depth w0
        prim(0, 16 * 8, 16 * 8, 16 * 20, 16 * 8, 40, 0xFFFFFF, sr.W_ONE, sr.W_ONE),            # none
        prim(9, 16 * 8, 16 * 8, 16 * 20, 16 * 8, 40, 0xFFFFFF, sr.W_ONE, sr.W_ONE),            # unknown
        prim(1, 16 * 12, 16 * 9, 0, 0, 0, 0x00FF00, 2000, 0),                                  # radius 0: the one pixel
        prim(1, 16 * 14, 16 * 9, 0, 0, -16, 0x00FF00, 2000, 0),                                # negative radius: nothing
        prim(2, -(1 << 30), 16 * 20, 1 << 30, 16 * 22, 12, 0x808000, 100000, 900000),          # saturates at +-2^20
        prim(2, 16 * 2, 16 * 30, 16 * (W - 3), 16 * 12 + 5, 24, 0xFF0000, 1 << 20, 1 << 29),   # crossing, rising towards b
        prim(2, 16 * 2, 16 * 12, 16 * (W - 3) + 7, 16 * 30, 24, 0x00FFFF, 1 << 29, 1 << 20),   # crossing, falling
        prim(1, 16 * 30, 16 * 6, 0, 0, 60, 0x123456, 777777, 0),                               # equal w: the later one wins
        prim(1, 16 * 33, 16 * 6, 0, 0, 60, 0x654321, 777777, 0),
        prim(2, 16 * 40 + 3, 16 * 3, 16 * 40 + 3, 16 * (H + 30), 9, 0xABCDEF, 1 << 28, 3),     # leaves through the bottom edge
    ], dtype=np.int32)


def plane_case(H, W, ortho):
    """A plane of points of ONE depth square to the camera, a capsule that passes through it (in front at one end, behind at
    the other), a disc of exactly the plane's w (primitive over point) and one a step behind it -> (view [1, 20], xyz [1, N,
    3], rgb, prims, the plane's w)"""
    fx = 10.0 if ortho else 30.0
    view = sr.look_at([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], fx, fx, W / 2.0, H / 2.0, NEAR, FAR, ortho)
    ys, zs = np.meshgrid(np.linspace(-8, 8, 2 * W), np.linspace(-5, 5, 2 * H))
    xyz = np.stack([np.full(ys.size, 2.0), ys.reshape(-1), zs.reshape(-1)], axis=1).astype(np.float32)[None]
    rgb = np.random.default_rng(3).integers(0, 256, size=xyz.shape, dtype=np.uint8)
    ok, _, _, q = sr.project(view, xyz[0])
    assert ok.all() and (q == q[0]).all()
    wp = int(q[0])
    prims = np.array([
        prim(2, 16 * 3, 16 * 4, 16 * (W - 4), 16 * (H - 5), 30, 0xFF00FF, wp + 5000, wp - 5000),
        prim(1, 16 * 10, 16 * (H - 8), 0, 0, 50, 0x00FF00, wp, 0),
        prim(1, 16 * 20, 16 * (H - 8), 0, 0, 50, 0x0000FF, wp - 1, 0),
    ], dtype=np.int32)
    return view[None], xyz, rgb, prims, wp


def identity_case():
    """A 24 x 40 depth map with depths in [1, 3], unprojected at the pixel centres through a camera -> (view [1, 20], xyz f32
    [1, 960, 3], rgb): rendered from that camera, pixel k shows point k"""
    H, W = 24, 40
    rng = np.random.default_rng(11)
    d = rng.uniform(1.0, 3.0, size=(H, W))
    fx, fy, cx, cy = 35.0, 33.0, 19.5, 12.25
    R = sr.look_at([0.3, -0.2, 0.1], [1.0, 0.5, 0.2], [0.0, 0.0, 1.0], fx, fy, cx, cy, 0.25, 8.0)
    M = R[:12].reshape(3, 4)
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    cam = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], axis=-1).reshape(-1, 3)
    world = (cam - M[:, 3]) @ M[:, :3]                          # R^T (c - t)
    rgb = rng.integers(0, 256, size=(1, H * W, 3), dtype=np.uint8)
    return R[None], world.astype(np.float32)[None], rgb, (H, W)


def skeleton_clip(T, J=17, seed=5):
    """world joints [T, J, 3] inside the reference's box (x, y in +-0.5, z in 0 .. 1.8), one NaN joint"""
    rng = np.random.default_rng(seed)
    j = np.stack([rng.uniform(-0.4, 0.4, (T, J)), rng.uniform(-0.4, 0.4, (T, J)), rng.uniform(0.1, 1.7, (T, J))], axis=-1)
    j[0, 3] = np.nan
    return j
