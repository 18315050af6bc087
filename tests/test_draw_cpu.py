"""CPU: the drawing rules' restatement has the properties the rules imply; the shape builders and the reference's drawing
functions build the right records on CPU tensors; the font table is well formed.  No device, no library call."""
import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_restated as dr
from skiing_analysis_pytorch_amd import bev, draw, geometry

FONT = geometry.font_5x7()
H, W = dc.SIZES[0]


def blank(value=50, ch=3):
    return np.full((H, W, ch), value, dtype=np.uint8)


def centre_distance(x, y):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.hypot(u - x, v - y)


# ---- the restatement's properties ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,y,r", [(30.0, 20.0, 7.0), (33.3125, 18.5625, 4.25), (2.0, 3.0, 6.0), (40.0, 20.0, 0.0)])
def test_disc_inside_and_outside(x, y, r):
    src = blank()
    out = dr.draw_frame(src, [dc.disc(x, y, r, 0x00FF8001)], FONT)
    x, y, r = dc.px(x) / 16, dc.px(y) / 16, dc.px(r) / 16
    d = centre_distance(x, y)
    assert (out[d > r + 1] == src[d > r + 1]).all()
    assert (out[d < r - 1] == np.array([0x01, 0x80, 0xFF], dtype=np.uint8)).all()
    if r >= 2:
        assert (d < r - 1).any() and (out != src).any()


def test_opacity_0_and_kind_0_change_nothing():
    src = dc.frames((), H, W, 3, seed=1)
    shapes = [dc.disc(30, 20, 8, opacity=0), dc.rec(dc.NONE, dc.px(30), dc.px(20), 0, 0, dc.px(8)), dc.capsule(3, 3, 60, 30, 4, opacity=0),
              dc.glyph("A", 10, 10, 2, opacity=0), dc.rec(9, dc.px(30), dc.px(20), 0, 0, dc.px(8))]
    assert (dr.draw_frame(src, shapes, FONT) == src).all()


def test_order_of_overlapping_half_opaque_shapes_matters():
    a, b = dc.overlap_pair()
    src = blank()
    assert (dr.draw_frame(src, a, FONT) != dr.draw_frame(src, b, FONT)).any()


def test_capsule_with_equal_ends_is_the_disc():
    src = dc.frames((), H, W, 3, seed=2)
    for x, y, t in ((30, 20, 6), (50.5, 10.25, 3), (0, 0, 9)):
        cap = dr.draw_frame(src, [dc.capsule(x, y, x, y, t, 0x00123456, 200)], FONT)
        dsc = dr.draw_frame(src, [dc.rec(dc.DISC, dc.px(x), dc.px(y), 0, 0, 8 * t, 0x00123456, 200)], FONT)
        assert (cap == dsc).all() and (cap != src).any()


def test_horizontal_capsule_is_symmetric_under_a_vertical_flip():
    src = blank(ch=1)
    yc = (H - 1) / 2          # the flip's axis: rows v and H - 1 - v
    for dy in (0.0, 3.25):
        up = dr.draw_frame(src, [dc.capsule(7.5, yc - dy, 55.25, yc - dy, 3)], FONT)
        down = dr.draw_frame(src, [dc.capsule(7.5, yc + dy, 55.25, yc + dy, 3)], FONT)
        assert (up[::-1] == down).all() and (up != src).any()


def test_saturated_coordinates_neither_overflow_nor_leave_their_box():
    big = 10 ** 7
    src = blank()
    with np.errstate(over="raise"):
        # far away: the boxes do not meet the frame
        far = [dc.rec(dc.DISC, big, big, 0, 0, 64), dc.rec(dc.DISC, -big, 300, 0, 0, 64), dc.rec(dc.CAPSULE, big, -big, big, big, 40),
               dc.rec(dc.GLYPH, -big, -big, ord("X"), 0, 3), dc.rec(dc.RING, big, big, 16, 0, 400)]
        assert (dr.draw_frame(src, far, FONT) == src).all()
        # a saturated diagonal crosses the frame as the line y = x and stays within its half width (2.5 px + 1)
        out = dr.draw_frame(src, [dc.rec(dc.CAPSULE, -big, -big, big, big, 40, 0x00FFFFFF)], FONT)
        v, u = np.nonzero((out != src).any(axis=-1))
        assert len(v) and (np.abs(u - v) / np.sqrt(2) <= 2.5 + 1).all()
        assert (out[np.arange(H), np.arange(H)] == 255).all()
        # a saturated end is the same as the end at 2^20
        a = dr.draw_frame(src, [dc.rec(dc.CAPSULE, 200, 200, big, 200, 16)], FONT)
        b = dr.draw_frame(src, [dc.rec(dc.CAPSULE, 200, 200, 1 << 20, 200, 16)], FONT)
        assert (a == b).all()


def test_glyph_cells_and_channel_3():
    src = blank(ch=4)
    out = dr.draw_frame(src, [dc.glyph(0x7F, 5, 6, 2, 0x00010203), dc.glyph(" ", 30, 6, 2), dc.glyph(3, 50, 6, 1, 0x00010203)], FONT)
    box = np.zeros((H, W), dtype=bool)
    box[6:20, 5:15] = True
    box[6:13, 50:55] = True       # a character outside the table is the filled box
    assert (out[box][:, :3] == [3, 2, 1]).all() and (out[~box] == src[~box]).all()
    assert (out[..., 3] == src[..., 3]).all()


# ---- the font ---------------------------------------------------------------------------------------------------------------
def test_font_table():
    assert FONT.shape == (96, 7) and FONT.dtype == np.uint8
    assert (FONT < 32).all()
    assert (FONT[0] == 0).all() and (FONT[95] == 31).all()
    printable = {FONT[i].tobytes() for i in range(95)}
    assert len(printable) == 95
    assert FONT[95].tobytes() not in printable
    assert all(FONT[i].any() for i in range(1, 95))


# ---- the builders -----------------------------------------------------------------------------------------------------------
def test_rounding_half_to_even_and_subpixel():
    xy = torch.tensor([[0.5, 1.5], [-0.5, 2.5], [3.49, -1.5], [7.0, 7.3125]], dtype=torch.float64)
    r = geometry.disc_shapes(xy, 4, (1, 2, 3))
    assert r.dtype == torch.int32 and tuple(r.shape) == (4, 8)
    assert r[:, 1:3].tolist() == [[0, 32], [0, 32], [48, -32], [112, 112]]
    assert (r[:, 0] == geometry.DRAW_DISC).all() and (r[:, 5] == 64).all() and (r[:, 6] == 0x030201).all() and (r[:, 7] == 256).all()
    s = geometry.disc_shapes(xy, 4.5, 7, subpixel=True)
    assert s[:, 1:3].tolist() == [[8, 24], [-8, 40], [56, -24], [112, 117]] and (s[:, 5] == 72).all() and (s[:, 6] == 0x070707).all()


def test_ring_and_segment_records():
    xy = torch.tensor([[10.0, 20.0]], dtype=torch.float64)
    ring = geometry.disc_shapes(xy, 5, (0, 255, 0), thickness=2, opacity=128)
    assert ring[0].tolist() == [geometry.DRAW_RING, 160, 320, 16, 0, 80, 0x00FF00, 128]
    seg = geometry.segment_shapes(xy, xy + 3.0, (255, 0, 0), 3)
    assert seg[0].tolist() == [geometry.DRAW_CAPSULE, 160, 320, 208, 368, 24, 0x0000FF, 256]
    poly = geometry.polyline_shapes(torch.tensor([[0.0, 0.0], [4.0, 0.0], [4.0, 4.0]], dtype=torch.float64), 9, 1, closed=True)
    assert poly[:, 1:5].tolist() == [[0, 0, 64, 0], [64, 0, 64, 64], [64, 64, 0, 0]]
    assert tuple(geometry.polyline_shapes(torch.zeros(2, 5, 2), 9, 1).shape) == (2, 4, 8)


def test_nan_and_valid_give_kind_0():
    xy = torch.tensor([[1.0, 2.0], [float("nan"), 2.0], [3.0, float("inf")], [4.0, 5.0]], dtype=torch.float64)
    r = geometry.disc_shapes(xy, 4, 255, valid=torch.tensor([True, True, True, False]))
    assert r[:, 0].tolist() == [geometry.DRAW_DISC, 0, 0, 0] and (r[1:] == 0).all()
    seg = geometry.segment_shapes(xy, xy.flip(0), 255, 1)
    assert seg[:, 0].tolist() == [geometry.DRAW_CAPSULE, 0, 0, geometry.DRAW_CAPSULE]


def test_text_shapes_advance_anchor_and_characters():
    anchor = torch.tensor([[10.0, 20.0], [float("nan"), 5.0], [3.5, 40.0]], dtype=torch.float64)
    r = geometry.text_shapes(["ab", "xyz", "é\x07~"], anchor, 2, (255, 255, 255))
    assert tuple(r.shape) == (8, 8)
    assert (r[[0, 1, 5, 6, 7], 0] == geometry.DRAW_GLYPH).all() and (r[2:5] == 0).all()
    assert r[:2, 1].tolist() == [160, 160 + 16 * 6 * 2]                        # six pixels a character and scale
    assert (r[:2, 2] == 16 * (20 - 13)).all()                                  # the cell's bottom row is the anchor's
    assert r[:2, 3].tolist() == [ord("a"), ord("b")] and (r[:2, 5] == 2).all()
    assert r[5:, 3].tolist() == [0x7F, 0x7F, ord("~")]                         # outside 0x20 .. 0x7F: the box
    assert r[5, 1].item() == 16 * 4                                            # 3.5 rounds to 4
    lead = geometry.text_shapes("hi", torch.zeros(2, 3, 1, 2), 1, 0)
    assert tuple(lead.shape) == (2, 3, 2, 8)


def test_number_shapes_are_str_of_device_integers():
    n = torch.tensor([0, 7, 10, 42, 99])
    r = geometry.number_shapes(n, torch.zeros(5, 2, dtype=torch.float64), 2, 1, 255).reshape(5, 2, 8)
    text = ["".join(chr(int(c)) for k, c in zip(row[:, 0], row[:, 3]) if k == geometry.DRAW_GLYPH) for row in r]
    assert text == ["0", "7", "10", "42", "99"]
    assert r[2, :, 1].tolist() == [0, 96] and (r[:, 0, 2] == -96).all()


def keypoint_records(F=3):
    k, s = dc.keypoints_17(F, H, W)
    return k, s, draw.keypoint_shapes(torch.from_numpy(k), scores=torch.from_numpy(s), score_thresh=0.5)


def test_draw_keypoints_record_count_and_order():
    k, s, rec = keypoint_records()
    F, K, E = k.shape[0], 17, len(draw.COCO_SKELETON)
    assert tuple(rec.shape) == (F, K + 2 * K + E, 8) and rec.dtype == torch.int32
    kinds = rec[..., 0].numpy()
    fin = np.isfinite(k).all(axis=-1)
    shown = fin & (s >= 0.5)
    # the points first: discs where the joint is finite and passes the score threshold
    assert ((kinds[:, :K] == geometry.DRAW_DISC) == shown).all() and (kinds[:, :K][~shown] == 0).all()
    assert (rec[:, :K, 6][torch.from_numpy(shown)] == 0x00FF00).all() and (rec[:, :K, 5][torch.from_numpy(shown)] == 64).all()
    assert rec[0, 0, 1:3].tolist() == [16 * 10, 16 * 12]                      # (10.5, 11.5): half to even
    # then the labels, white, numbering the joints that pass the filter in order (the reference's enumerate)
    labels = rec[:, K:3 * K].reshape(F, K, 2, 8).numpy()
    for f in range(F):
        number = np.cumsum(s[f] >= 0.5) - 1
        for j in range(K):
            text = "".join(chr(c) for kind, c in zip(labels[f, j, :, 0], labels[f, j, :, 3]) if kind == geometry.DRAW_GLYPH)
            assert text == (str(number[j]) if shown[f, j] else "")
    assert (labels[..., 6][labels[..., 0] == geometry.DRAW_GLYPH] == 0xFFFFFF).all()
    j = int(np.argmax(shown[1]))
    assert labels[1, j, 0, 1] == 16 * (round(k[1, j, 0]) + 4) and labels[1, j, 0, 2] == 16 * (round(k[1, j, 1]) - 4 - 6)
    # then the edges: both ends finite, whatever the scores
    edges = kinds[:, 3 * K:]
    for e, (a, b) in enumerate(draw.COCO_SKELETON):
        assert ((edges[:, e] == geometry.DRAW_CAPSULE) == (fin[:, a] & fin[:, b])).all()
    assert (edges[edges != geometry.DRAW_CAPSULE] == 0).all() and (edges == 0).any()
    live = rec[:, 3 * K:][torch.from_numpy(edges == geometry.DRAW_CAPSULE)]
    assert (live[:, 5] == 16).all() and (live[:, 6] == 0xFFFF00).all()


def test_draw_keypoints_options():
    k, s = dc.keypoints_17(2, H, W)
    kt = torch.from_numpy(k)
    assert tuple(draw.keypoint_shapes(kt, with_index=False, skeleton=None).shape) == (2, 17, 8)
    assert tuple(draw.keypoint_shapes(kt, skeleton=[(0, 1), (2, 40)]).shape) == (2, 17 * 3 + 1, 8)
    rings = draw.keypoint_shapes(kt, thickness=1, with_index=False, skeleton=None)
    assert set(rings[..., 0].unique().tolist()) == {0, geometry.DRAW_RING}
    with pytest.raises(ValueError):
        draw.keypoint_shapes(kt, scores=torch.zeros(2, 5), score_thresh=0.5)


def test_reprojection_shapes_and_stats():
    obs, rep = dc.reprojection(3, 6, H, W)
    names = ["nose", "eye"]
    rec = draw.reprojection_shapes(torch.from_numpy(obs), torch.from_numpy(rep), W, H, names)
    L = 4
    assert tuple(rec.shape) == (3, 6 * (3 + L), 8)
    r = rec.reshape(3, 6, 3 + L, 8).numpy()
    ok = np.isfinite(obs).all(-1) & np.isfinite(rep).all(-1)
    assert not ok.all() and ((r[:, :, 0, 0] == geometry.DRAW_RING) == ok).all() and (r[~ok] == 0).all()
    assert (r[ok][:, :3, 0] == [geometry.DRAW_RING, geometry.DRAW_RING, geometry.DRAW_CAPSULE]).all()
    assert (r[ok][:, :3, 6] == [0x00FF00, 0xFF0000, 0x00FFFF]).all()
    assert (r[ok][:, 1, 1] <= 16 * (W - 1)).all() and (r[:, 1, 1, 1] == 16 * (W - 1)).all()       # _clip_xy
    text = ["".join(chr(c) for kind, c in zip(row[3:, 0], row[3:, 3]) if kind == geometry.DRAW_GLYPH) for row in r[1]]
    assert text == ["nose", "eye", "2", "3", "4", "5"]
    got = draw.reprojection_stats(torch.from_numpy(obs), torch.from_numpy(rep)).numpy()
    want = dr.reprojection_stats(obs, rep)
    assert np.isfinite(want).all() and (np.abs(got - want) <= 1e-9 * (1 + np.abs(want))).all()


def test_point_shapes():
    pts = torch.tensor([[10.9, 20.2], [-3.7, 5.0], [float("nan"), 1.0]], dtype=torch.float64)
    rec = bev.point_shapes(pts, (0, 0, 255), radius=4)
    assert tuple(rec.shape) == (3 + 3, 8)
    assert rec[:3, 0].tolist() == [geometry.DRAW_DISC, geometry.DRAW_DISC, 0]
    assert rec[:2, 1:3].tolist() == [[160, 320], [-48, 80]]                   # truncated towards zero, as np.int32
    assert rec[3:, 3].tolist() == [ord("1"), ord("2"), 0] and rec[3, 5].item() == 2 and rec[3, 6].item() == 0xFF0000
    assert rec[3, 1:3].tolist() == [16 * 18, 16 * (12 - 13)]
    named = bev.point_shapes(pts[:2], labels=["ab", "c"])
    assert tuple(named.shape) == (2 + 3, 8)


def test_cat_shapes_repeats_shared_lists():
    a, b = torch.zeros(4, 8, dtype=torch.int32), torch.ones(2, 3, 5, 8, dtype=torch.int32)
    c = geometry.cat_shapes(a, b)
    assert tuple(c.shape) == (2, 3, 9, 8) and c.is_contiguous() and (c[..., :4, :] == 0).all() and (c[..., 4:, :] == 1).all()
