"""GPU: the rasteriser (csrc/draw.hip) against the NumPy restatement (tests/draw_restated.py), byte for byte, on frames that
divide no tile and whose rows are not dword-aligned, in every layout; and the reference's drawing functions on top of it."""
import functools

import numpy as np
import pytest
import torch

import draw_cases as dc
import draw_restated as dr
from skiing_analysis_pytorch_amd import _lib, bev, draw, geometry

pytestmark = pytest.mark.gpu

FONT = geometry.font_5x7()
# (leading axes, (H, W), channels): 3 W and W are no multiples of 4 in either size
LAYOUTS = {"F3": ((2,), dc.SIZES[0], 3), "F1": ((1,), dc.SIZES[1], 1), "CF4": ((2, 3), dc.SIZES[1], 4), "CF3": ((2, 3), dc.SIZES[0], 3)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def clip(layout):
    lead, (H, W), ch = LAYOUTS[layout]
    return dc.frames(lead, H, W, ch, seed=len(lead) * 10 + ch)


def check(frames, shapes, **kw):
    """draw on the device, twice: equal to the restatement, the rerun bitwise identical, the input untouched"""
    fd, sd = dev(frames), dev(shapes)
    got = geometry.draw_shapes(fd, sd, **kw)
    again = geometry.draw_shapes(fd, sd, **kw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == frames.shape
    assert torch.equal(fd.cpu(), torch.from_numpy(frames)), "the input was modified"
    want = dr.draw_clip(frames, shapes, FONT)
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert not len(bad), f"{len(bad)} bytes differ from the restatement, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    assert torch.equal(got, again)
    return fd, sd, got, want


CASE_NAMES = sorted(dc.cases(*dc.SIZES[0]))


@pytest.mark.parametrize("layout", ["F3", "CF4", "F1"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_restatement(name, layout):
    frames = clip(layout)
    H, W = LAYOUTS[layout][1]
    shapes = dc.cases(H, W)[name]
    _, _, _, want = check(frames, shapes)
    if name not in ("kinds",):
        assert (want != frames).any(), "the case draws nothing"


@pytest.mark.parametrize("layout", ["F3", "F1"])
@pytest.mark.parametrize("n", dc.COUNTS)
def test_list_lengths_across_the_seams(n, layout):
    H, W = LAYOUTS[layout][1]
    check(clip(layout), dc.counted(n, H, W))


def test_no_shapes_is_a_copy():
    for layout in ("F3", "CF4"):
        frames = clip(layout)
        fd = dev(frames)
        got = geometry.draw_shapes(fd, torch.zeros((0, 8), dtype=torch.int32, device="cuda"))
        assert got.data_ptr() != fd.data_ptr() and torch.equal(got, fd)
        same = geometry.draw_shapes(fd, torch.zeros((0, 8), dtype=torch.int32, device="cuda"), inplace=True)
        assert same.data_ptr() == fd.data_ptr() and torch.equal(fd.cpu(), torch.from_numpy(frames))


def test_300_shapes_on_one_tile():
    shapes = dc.one_tile(300)
    _, _, _, want = check(clip("F3"), shapes)
    frames = clip("F3")
    assert (want[:, :16, :64] != frames[:, :16, :64]).any()


@pytest.mark.parametrize("axes", ["shared", "per_frame", "per_camera"])
def test_shape_tensor_layouts(axes):
    frames = clip("CF3")
    H, W = LAYOUTS["CF3"][1]
    C, F = frames.shape[:2]
    if axes == "shared":
        shapes = dc.random_shapes(40, H, W, seed=11)
    elif axes == "per_frame":
        shapes = np.stack([dc.random_shapes(40, H, W, seed=20 + f) for f in range(F)])
    else:
        shapes = np.stack([np.stack([dc.random_shapes(40, H, W, seed=30 + 7 * c + f) for f in range(F)]) for c in range(C)])
    check(frames, shapes)
    # four-axis frames take [P, 8] and [F, P, 8]
    if axes != "per_camera":
        check(frames[1], shapes)


def test_order_of_two_overlapping_shapes():
    a, b = dc.overlap_pair()
    frames = clip("F3")
    _, _, ga, _ = check(frames, a)
    _, _, gb, _ = check(frames, b)
    assert not torch.equal(ga, gb)


def test_frame_alone_equals_frame_in_batch_and_inplace_equals_out_of_place():
    frames = clip("CF4")
    H, W = LAYOUTS["CF4"][1]
    C, F = frames.shape[:2]
    shapes = np.stack([np.stack([dc.random_shapes(70, H, W, seed=50 + 5 * c + f) for f in range(F)]) for c in range(C)])
    fd, sd, got, _ = check(frames, shapes)
    for c in range(C):
        for f in range(F):
            alone = geometry.draw_shapes(fd[c, f][None].contiguous(), sd[c, f].contiguous())
            assert torch.equal(alone[0], got[c, f])
    assert torch.equal(got[..., 3], fd[..., 3]), "channel 3 of a 4-channel clip was written"
    assert not torch.equal(got[..., :3], fd[..., :3])
    work = fd.clone()
    res = geometry.draw_shapes(work, sd, inplace=True)
    assert res.data_ptr() == work.data_ptr() and torch.equal(work, got)
    out = torch.empty_like(fd)
    assert geometry.draw_shapes(fd, sd, out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)


def test_custom_font_is_data():
    font = np.zeros((96, 7), dtype=np.uint8)
    font[ord("A") - 0x20] = [1, 2, 4, 8, 16, 8, 4]
    frames = clip("F3")
    shapes = np.array([dc.glyph("A", 5, 5, 3), dc.glyph("B", 30, 5, 3)], dtype=np.int32)
    got = geometry.draw_shapes(dev(frames), dev(shapes), font=dev(font)).cpu().numpy()
    assert (got == dr.draw_clip(frames, shapes, font)).all() and (got != frames).any()


# ---- the reference's functions -----------------------------------------------------------------------------------------------
def test_draw_keypoints():
    frames = clip("CF3")
    (C, F), (H, W) = frames.shape[:2], LAYOUTS["CF3"][1]
    k, s = dc.keypoints_17(C * F, H, W)
    k, s = k.reshape(C, F, 17, 2), s.reshape(C, F, 17)
    assert np.isnan(k).any(axis=-1).sum(axis=-1).min() == 2
    fd = dev(frames)
    got = draw.draw_keypoints(fd, dev(k), scores=dev(s), score_thresh=0.5)
    shapes = draw.keypoint_shapes(torch.from_numpy(k), scores=torch.from_numpy(s), score_thresh=0.5).numpy()     # the builders, on the host
    want = dr.draw_clip(frames, shapes, FONT)
    assert (got.cpu().numpy() == want).all() and (want != frames).any()
    assert torch.equal(fd.cpu(), torch.from_numpy(frames))
    assert torch.equal(got, draw.draw_keypoints(fd, dev(k), scores=dev(s), score_thresh=0.5))
    # a four-axis clip, rings, no labels
    got1 = draw.draw_keypoints(fd[0], dev(k[0]), thickness=1, with_index=False)
    want1 = dr.draw_clip(frames[0], draw.keypoint_shapes(torch.from_numpy(k[0]), thickness=1, with_index=False).numpy(), FONT)
    assert (got1.cpu().numpy() == want1).all()


@pytest.mark.parametrize("titles", [False, True])
def test_render_reprojection_panel(titles):
    F, J = 2, 6
    (H1, W1), (H2, W2) = dc.SIZES
    img1, img2 = dc.frames((F,), H1, W1, 3, seed=1), dc.frames((F,), H2, W2, 3, seed=2)
    oL, rL = dc.reprojection(F, J, H1, W1, seed=5)
    oR, rR = dc.reprojection(F, J, H2, W2, seed=6)
    names = ["nose", "l_eye"]
    visL, visR, panel = draw.render_reprojection_panel(dev(img1), dev(img2), dev(oL), dev(oR), dev(rL), dev(rR), joint_names=names, titles=titles)
    assert tuple(panel.shape) == (F, max(H1, H2), W1 + W2, 3) and panel.dtype == torch.uint8
    wantL = dr.draw_clip(img1, draw.reprojection_shapes(torch.from_numpy(oL), torch.from_numpy(rL), W1, H1, names).numpy(), FONT)
    wantR = dr.draw_clip(img2, draw.reprojection_shapes(torch.from_numpy(oR), torch.from_numpy(rR), W2, H2, names).numpy(), FONT)
    assert (visL.cpu().numpy() == wantL).all() and (visR.cpu().numpy() == wantR).all() and (wantL != img1).any()
    # the title numbers, computed on the device
    for o, r in ((oL, rL), (oR, rR)):
        got, want = draw.reprojection_stats(dev(o), dev(r)).cpu().numpy(), dr.reprojection_stats(o, r)
        assert np.isfinite(want).all() and (np.abs(got - want) <= 1e-9 * (1 + np.abs(want))).all()
    p = panel.cpu().numpy()
    if not titles:
        assert (p[:, :H1, :W1] == wantL).all() and (p[:, :H2, W1:] == wantR).all() and (p[:, H2:, W1:] == 0).all()
        return
    # with titles: the two halves are the views with their title line drawn over them
    line = "{} | RMSE={:.2f}px  (mean={:.2f}, med={:.2f}, max={:.2f})"
    base = np.zeros_like(p)
    base[:, :H1, :W1], base[:, :H2, W1:] = wantL, wantR
    for f in range(F):
        sl, sr = dr.reprojection_stats(oL[f], rL[f]), dr.reprojection_stats(oR[f], rR[f])
        text = torch.cat([geometry.text_shapes(line.format(draw.TITLE_LEFT, *sl), torch.tensor([[20.0, 30.0]]), 2, (255, 255, 255)),
                          geometry.text_shapes(line.format(draw.TITLE_RIGHT, *sr), torch.tensor([[W1 + 20.0, 30.0]]), 2, (255, 255, 255))])
        assert (p[f] == dr.draw_frame(base[f], text.numpy(), FONT)).all()
    assert (p != base).any()


def test_bev_draw_points():
    frames = clip("F3")
    H, W = LAYOUTS["F3"][1]
    pts = np.array([[10.9, 20.2], [-3.7, 5.0], [np.nan, 1.0], [W - 2.5, H - 1.0]])
    got = bev.draw_points(dev(frames), dev(pts), (0, 0, 255), radius=4)
    want = dr.draw_clip(frames, bev.point_shapes(torch.from_numpy(pts), (0, 0, 255), 4).numpy(), FONT)
    assert (got.cpu().numpy() == want).all() and (want != frames).any()
    per_frame = np.stack([pts, pts + 3.0])
    got2 = bev.draw_points(dev(frames), dev(per_frame), (9, 8, 7), radius=2, labels=["a", "b", "c", "d"])
    want2 = dr.draw_clip(frames, bev.point_shapes(torch.from_numpy(per_frame), (9, 8, 7), 2, ["a", "b", "c", "d"]).numpy(), FONT)
    assert (got2.cpu().numpy() == want2).all()


# ---- error paths -------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_bad_arguments():
    fd = dev(clip("F3"))
    ok = dev(dc.counted(1, 40, 72))
    with pytest.raises(_lib.SkimiError):
        geometry.draw_shapes(fd.cpu(), ok)
    with pytest.raises(_lib.SkimiError):
        geometry.draw_shapes(fd, ok.cpu())
    with pytest.raises(_lib.SkimiError):
        geometry.draw_shapes(fd.float(), ok)
    with pytest.raises(ValueError):
        geometry.draw_shapes(fd, ok.long())
    with pytest.raises(ValueError):
        geometry.draw_shapes(fd, torch.zeros((geometry.DRAW_MAX_SHAPES + 1, 8), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        geometry.draw_shapes(fd, torch.zeros((3, 5, 8), dtype=torch.int32, device="cuda"))       # F is 2
    with pytest.raises(ValueError):
        geometry.draw_shapes(fd, ok, font=torch.zeros((95, 7), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        geometry.draw_shapes(fd[:, :, :, :2], ok)
    with pytest.raises(_lib.SkimiError):
        draw.draw_keypoints(fd, torch.zeros(2, 17, 2))


def test_c_entry_reports_errors_without_a_launch():
    lib, st = _lib.lib(), _lib.current_stream()
    fd = dev(clip("F3"))
    before = fd.clone()
    out, sh, font = torch.empty_like(fd), dev(dc.counted(1, 40, 72)), dev(FONT)
    F, H, W, ch = fd.shape
    good = [fd.data_ptr(), out.data_ptr(), sh.data_ptr(), 2, font.data_ptr(), 1, F, H, W, ch, 1, st]

    def call(**change):
        names = ["frames", "out", "shapes", "axes", "font", "C", "F", "H", "W", "ch", "P", "stream"]
        return lib.skimi_draw_shapes_u8(*[change.get(n, v) for n, v in zip(names, good)])

    out.fill_(7)
    for change, word in ((dict(frames=None), b"NULL"), (dict(out=None), b"NULL"), (dict(shapes=None), b"NULL"), (dict(font=None), b"NULL"),
                         (dict(ch=2), b"channels"), (dict(P=geometry.DRAW_MAX_SHAPES + 1), b"P ="), (dict(P=-1), b"P ="),
                         (dict(F=0), b"C ="), (dict(H=0), b"frame"), (dict(W=0), b"frame"), (dict(axes=5), b"shape_axes")):
        assert call(**change) != 0, change
        assert word in lib.skimi_last_error(), (change, lib.skimi_last_error())
    torch.cuda.synchronize()
    assert (out == 7).all() and torch.equal(fd, before)
    assert call() == 0
    assert (out.cpu().numpy() == dr.draw_clip(before.cpu().numpy(), sh.cpu().numpy(), FONT)).all()
