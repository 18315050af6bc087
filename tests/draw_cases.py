"""Inputs of the drawing tests (tests/test_draw_cpu.py, tests/test_draw_gpu.py): frames that divide neither a 64 x 16 nor a
32 x 32 tile and whose 3 W is no multiple of 4, and shape lists for every rule and seam of the rasteriser."""
import numpy as np

SIZES = ((40, 72), (33, 70))      # H, W
MAX_SHAPES = 1024
NONE, DISC, RING, CAPSULE, GLYPH = 0, 1, 2, 3, 4


def px(v):
    """pixels -> sixteenths"""
    return int(round(16 * v))


def rec(kind, x0, y0, x1=0, y1=0, r=0, colour=0x00C08040, opacity=256):
    return [kind, x0, y0, x1, y1, r, colour, opacity]


def disc(x, y, r, colour=0x0020E0A0, opacity=256):
    return rec(DISC, px(x), px(y), 0, 0, px(r), colour, opacity)


def ring(x, y, r, thickness, colour=0x00F04010, opacity=256):
    return rec(RING, px(x), px(y), 8 * thickness, 0, px(r), colour, opacity)


def capsule(xa, ya, xb, yb, thickness, colour=0x0010C0F0, opacity=256):
    return rec(CAPSULE, px(xa), px(ya), px(xb), px(yb), 8 * thickness, colour, opacity)


def glyph(ch, left, top, scale, colour=0x00FFFFFF, opacity=256):
    return rec(GLYPH, px(left), px(top), ch if isinstance(ch, int) else ord(ch), 0, scale, colour, opacity)


def frames(lead, H, W, ch, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (*lead, H, W, ch), dtype=np.uint8)


def random_shapes(n, H, W, seed, x_hi=None, y_hi=None):
    """n records of all kinds (kind 0 among them) spread over [-8, x_hi + 8] x [-8, y_hi + 8] pixels, at sub-pixel positions"""
    rng = np.random.default_rng(seed)
    x_hi, y_hi = W if x_hi is None else x_hi, H if y_hi is None else y_hi
    out = np.zeros((n, 8), dtype=np.int32)
    for i in range(n):
        kind = int(rng.integers(0, 5))
        x0, y0 = int(rng.integers(-128, 16 * x_hi + 128)), int(rng.integers(-128, 16 * y_hi + 128))
        colour, opacity = int(rng.integers(0, 1 << 24)), int(rng.choice([40, 128, 200, 256]))
        if kind == GLYPH:
            out[i] = rec(kind, x0, y0, int(rng.integers(0x20, 0x80)), 0, int(rng.integers(1, 3)), colour, opacity)
        elif kind == RING:
            out[i] = rec(kind, x0, y0, int(rng.integers(0, 33)), 0, int(rng.integers(0, 160)), colour, opacity)
        else:
            x1, y1 = x0 + int(rng.integers(-400, 401)), y0 + int(rng.integers(-400, 401))
            out[i] = rec(kind, x0, y0, x1, y1, int(rng.integers(0, 64)), colour, opacity)
    return out


def overlap_pair():
    """two lists whose only difference is the order of two overlapping half-opaque shapes"""
    a, b = disc(30, 18, 9, 0x000000FF, 128), capsule(20, 10, 44, 26, 6, 0x0000FF00, 128)
    base = [ring(10, 10, 5, 2)]
    return np.array(base + [a, b], dtype=np.int32), np.array(base + [b, a], dtype=np.int32)


def cases(H, W):
    """name -> int32 [P, 8]"""
    big = 10 ** 7
    c = {
        "disc": [disc(20, 12, 6), disc(50.5, 20.25, 3.5, 0x00804020, 200)],
        "ring": [ring(22, 14, 8, 2), ring(48.25, 25.5, 5, 1, 0x0040FF40, 180), ring(36, 20, 12, 0)],
        "capsule": [capsule(5, 5, 60, 30, 2), capsule(30.5, 3.25, 12.75, 31, 1, 0x00FF8000, 150)],
        "glyph": [glyph("A", 4, 4, 1), glyph("g", 12, 6, 2, 0x0000FFFF), glyph(0x7F, 30, 3, 1), glyph(5, 40, 3, 1), glyph("~", 50, 20, 1)],
        # centred on (64, 16) and (32, 32): the corner of four 64 x 16 tiles, and of four 32 x 32 ones
        "corner": [disc(64, 16, 6), ring(64, 16, 9, 2), capsule(58, 10, 70, 22, 2), glyph("W", 62, 13, 1), disc(32, 32, 5, 0x00FF00FF, 128),
                   disc(63.5, 15.5, 2, 0x00FFFFFF)],
        "outside": [disc(-3, 10, 6), disc(W + 2, 20, 5), disc(30, -2, 4), disc(30, H + 1, 4), disc(-50, -50, 8), disc(W + 80, H + 80, 8),
                    capsule(-20, 20, 10, 20, 2), capsule(W - 5, H - 5, W + 30, H + 30, 3), ring(W, H, 10, 2), ring(-400, 10, 20, 2),
                    glyph("Q", -3, -3, 1), glyph("Q", W + 5, 5, 1)],
        "long": [capsule(-5000, -5000, 5000, 5000, 2), capsule(-5000, 4000, 5000, -3900, 1, 0x00FFFF00, 128)],
        "segments": [capsule(3, 8, 60, 8, 1), capsule(10, 2, 10, 38, 2), capsule(5, 5, 30, 30, 1), capsule(40, 2, 43, 37, 1),
                     capsule(66, 30, 20, 28, 3, 0x00A0A0A0, 100)],
        "radius0": [disc(10, 10, 0), capsule(15, 5, 50, 25, 0), ring(30, 20, 0, 0), ring(45, 20, 6, 0), rec(DISC, px(60), px(10), 0, 0, -8),
                    rec(DISC, px(60), px(20), 0, 0, -7), rec(DISC, px(20), px(30), 0, 0, -100)],
        "opacity": [disc(20, 20, 10, 0x00FFFFFF, 0), disc(35, 20, 10, 0x00FFFFFF, 128), disc(50, 20, 10, 0x00FFFFFF, 256),
                    disc(42, 20, 6, 0x00000000, 128), rec(DISC, px(10), px(10), 0, 0, px(5), 0x00FFFFFF, 1000),
                    rec(DISC, px(10), px(30), 0, 0, px(5), 0x00FFFFFF, -5)],
        "glyph_scales": [glyph("R", 2, 2, 1), glyph("k", 10, 2, 3), glyph("8", W - 8, 10, 3), glyph("M", 20, H - 10, 3), glyph("j", -2, -4, 3),
                         glyph("@", W - 3, H - 4, 1), rec(GLYPH, px(40), px(2), ord("S"), 0, 0), rec(GLYPH, px(48), px(2), ord("S"), 0, -3)],
        "saturated": [rec(DISC, big, big, 0, 0, 64), rec(DISC, -big, -big, 0, 0, 64), rec(CAPSULE, -big, -big, big, big, 40),
                      rec(CAPSULE, -big, big, big, -big, 16, 0x0000FF00, 128), rec(RING, 16 * 30, 16 * 20, big, 0, big, 0x00FF0000, 64),
                      rec(DISC, 16 * 30, 16 * 20, 0, 0, big, 0x000000FF, 32), rec(GLYPH, -big, -big, ord("X"), 0, big),
                      rec(RING, big, 100, -big, 0, -big), rec(CAPSULE, 200, 200, big, 200, 16)],
        "kinds": [rec(NONE, px(20), px(20), 0, 0, px(10)), rec(7, px(20), px(20), 0, 0, px(10)), rec(-1, px(20), px(20), 0, 0, px(10)),
                  disc(40, 20, 4)],
        "capsule_point": [capsule(30, 20, 30, 20, 6), capsule(50.5, 10.25, 50.5, 10.25, 3)],
    }
    return {k: np.array(v, dtype=np.int32).reshape(-1, 8) for k, v in c.items()}


COUNTS = (1, 64, 65, 257, MAX_SHAPES)      # across the ballot (64) and chunk (256) seams of the tile list


def counted(n, H, W):
    return random_shapes(n, H, W, seed=1000 + n)


def one_tile(n=300):
    """n shapes that all lie on the first 64 x 16 tile"""
    return random_shapes(n, 16, 64, seed=7, x_hi=40, y_hi=10)


def keypoints_17(F, H, W, seed=3):
    """[F, 17, 2] float64 pixels inside the frame with two NaN joints per frame, and scores [F, 17] of which some fall below 0.5"""
    rng = np.random.default_rng(seed)
    k = np.stack([rng.uniform(2, W - 3, (F, 17)), rng.uniform(2, H - 3, (F, 17))], axis=-1)
    for f in range(F):
        k[f, (3 + f) % 17, 0] = np.nan
        k[f, (11 + 2 * f) % 17] = np.nan
    k[0, 0] = [10.5, 11.5]       # ties: half to even
    s = rng.uniform(0.2, 1.0, (F, 17))
    return k, s


def reprojection(F, J, H, W, seed=5):
    """observed [F, J, 2] and reprojected [F, J, 2] points: a NaN joint, and reprojections outside the frame"""
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.uniform(3, W - 4, (F, J)), rng.uniform(3, H - 4, (F, J))], axis=-1)
    rep = obs + rng.normal(0, 4.0, obs.shape)
    rep[:, 1] += [W, 0]          # clipped to the frame
    obs[0, 2] = np.nan
    rep[F - 1, 0, 1] = np.nan
    return obs, rep
