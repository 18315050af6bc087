"""GPU: the mask analysis kernels (csrc/masks.hip) against the NumPy restatement (tests/masks_restated.py), bit for bit, on
images that divide no tile, whose pixel count is no multiple of 64 and whose rows are not dword-aligned, and on the one-pixel,
one-row and one-column images; the reference's names (the package's masks.py) on top of them.  Everything compared is an
integer, or a float made by one stated operation from integers: there is no tolerance anywhere."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import masks_cases as mc
import masks_restated as mr
from skiing_analysis_pytorch_amd import bev, geometry, masks

pytestmark = pytest.mark.gpu

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "masks.npz")
ALL_SIZES = mc.SIZES + mc.DEGENERATE
COMPONENT_CASES = [(name, size) for size in ALL_SIZES for name in sorted(mc.component_cases(*size))]   # no rings below 12 pixels a side
EDT_NAMES = sorted(mc.edt_cases(*mc.SIZES[0]))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same(got, want, what):
    g = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert g.dtype == want.dtype and g.shape == want.shape, f"{what}: {g.dtype} {g.shape} against {want.dtype} {want.shape}"
    if g.dtype.kind == "f":
        g, want = g.view(np.uint32 if g.itemsize == 4 else np.uint64), want.view(np.uint32 if want.itemsize == 4 else np.uint64)
    bad = np.argwhere(g != want)
    assert not len(bad), f"{what}: {len(bad)} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def same_results(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@functools.lru_cache(maxsize=None)
def components_want(size, name, connectivity, maxc):
    return mr.components_batch(mc.batch(mc.component_cases(*size)[name]), connectivity, maxc)


@functools.lru_cache(maxsize=None)
def edt_want(size, name):
    m, border = mc.edt_cases(*size)[name]
    d2 = np.stack([mr.edt_d2(k, border) for k in mc.batch(m)])
    return d2, mr.edt_dist(d2)


# ---- components ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name,size", COMPONENT_CASES)
def test_components_equal_restatement(name, size, connectivity):
    cases = mc.component_cases(*size)
    maxc = mc.MANY_MAX_COMPONENTS if name == "many" else 256
    m = mc.batch(cases[name])
    md = dev(m)
    got = geometry.mask_components(md, connectivity, maxc)
    again = geometry.mask_components(md, connectivity, maxc)
    assert torch.equal(md.cpu(), torch.from_numpy(m)), "the input was modified"
    for field, want in zip(got._fields, components_want(size, name, connectivity, maxc)):
        same(getattr(got, field), want, f"{name} {field}")
    same_results(got, again)
    if name == "many" and size != (1, 1):
        assert int(got.count.min()) > maxc and bool((got.stats[..., 0] > 0).all())


@pytest.mark.parametrize("name", ["serpentine", "random_0.5", "rings", "many"])
def test_components_alone_in_a_batch_bool_and_no_table(name):
    size = mc.SIZES[1]
    m = mc.batch(mc.component_cases(*size)[name])
    md = dev(m)
    got = geometry.mask_components(md, 8, 16)
    for b in range(mc.B):
        alone = geometry.mask_components(md[b], 8, 16)
        assert alone.labels.dim() == 2 and alone.count.dim() == 0 and tuple(alone.stats.shape) == (16, 7)
        same_results(alone, [f[b] for f in got])
    same_results(geometry.mask_components(md != 0, 8, 16), got)
    same_results(geometry.mask_components(md * 255, 8, 16), got)
    bare = geometry.mask_components(md, 8, 0)
    assert tuple(bare.stats.shape) == (mc.B, 0, 7)
    same_results(bare[:3], got[:3])


def test_components_on_tile_borders():
    """every way two tiles can touch: a diagonal pair across a corner of four 64 x 16 tiles, pairs across each border"""
    H, W = 40, 140
    m = np.zeros((4, H, W), dtype=np.uint8)
    m[0, 15, 63] = m[0, 16, 64] = 1                    # across the corner, down-right
    m[1, 15, 64] = m[1, 16, 63] = 1                    # across the corner, down-left
    m[2, 10, 63] = m[2, 11, 64] = m[2, 20, 64] = m[2, 21, 63] = 1      # diagonals across a vertical border only
    m[3, 15, 30] = m[3, 16, 31] = m[3, 31, 100] = m[3, 32, 99] = 1     # diagonals across a horizontal border only
    for connectivity in (4, 8):
        got = geometry.mask_components(dev(m), connectivity, 4)
        for field, want in zip(got._fields, mr.components_batch(m, connectivity, 4)):
            same(getattr(got, field), want, f"borders {connectivity} {field}")
    assert host(geometry.mask_components(dev(m), 8, 0).count).tolist() == [1, 1, 2, 2]


# ---- distance transform ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ALL_SIZES)
@pytest.mark.parametrize("name", EDT_NAMES)
def test_distance_transform_equals_restatement(name, size):
    m, border = mc.edt_cases(*size)[name]
    m = mc.batch(m)
    md = dev(m)
    got = geometry.distance_transform(md, border)
    again = geometry.distance_transform(md, border)
    assert torch.equal(md.cpu(), torch.from_numpy(m)), "the input was modified"
    d2, dist = edt_want(size, name)
    same(got.d2, d2, f"{name} d2")
    same(got.dist, dist, f"{name} dist")
    same_results(got, again)
    if name == "no_zero":
        assert bool((got.d2 == geometry.EDT_NONE).all()) and bool(torch.isinf(got.dist).all())
    same_results(geometry.distance_transform(md != 0, border), got)
    alone = geometry.distance_transform(md[1], border)
    same_results(alone, [got.d2[1], got.dist[1]])


@pytest.mark.parametrize("border", [False, True])
def test_inner_point_equals_restatement(border):
    H, W = mc.SIZES[0]
    cases = mc.edt_cases(H, W)
    names = [n for n in sorted(cases) if cases[n][1] == border]
    m = np.stack([cases[n][0] for n in names] + [mc.two_maxima(H, W), np.zeros((H, W), dtype=np.uint8)])
    md = dev(m)
    xy, d2 = geometry.mask_inner_point(md, border)
    want = [mr.inner_point(k, border) for k in m]
    same(xy, np.array([w[0] for w in want], dtype=np.int32), "inner point xy")
    same(d2, np.array([w[1] for w in want], dtype=np.int32), "inner point d2")
    assert host(xy)[-2].tolist() == [43, 13] and host(xy)[-1].tolist() == [0, 0] and int(d2[-1]) == 0
    same_results(geometry.mask_inner_point(md, border), (xy, d2))
    one = geometry.mask_inner_point(md[-2] != 0, border)
    assert tuple(one[0].shape) == (2,) and one[1].dim() == 0
    same_results(one, (xy[-2], d2[-2]))
    assert torch.equal(md.cpu(), torch.from_numpy(m))


# ---- boxes and IoU ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ALL_SIZES)
def test_boxes_equal_restatement(size):
    cases = mc.component_cases(*size)
    m = np.stack([cases[n] for n in sorted(cases)])
    md = dev(m)
    got = geometry.mask_boxes(md)
    xyxy, area = mr.boxes(m)
    same(got.xyxy, xyxy, "xyxy")
    same(got.area, area, "area")
    empty = sorted(cases).index("empty")
    assert host(got.xyxy)[empty].tolist() == [size[1], size[0], 0, 0]
    same_results(geometry.mask_boxes(md), got)
    same_results(geometry.mask_boxes(md != 0), got)
    same_results(geometry.mask_boxes(md[3]), [got.xyxy[3], got.area[3]])
    same(masks.masks_to_boxes(md), xyxy.astype(np.float32), "masks_to_boxes")
    assert torch.equal(md.cpu(), torch.from_numpy(m))


@pytest.mark.parametrize("k", range(len(mc.IOU_SHAPES)))
def test_iou_equals_restatement_and_reference(k):
    n, m = mc.IOU_SHAPES[k]
    a, b = GOLD[f"iou{k}_a"], GOLD[f"iou{k}_b"]
    ad, bd = dev(a), dev(b)
    got = geometry.mask_iou(ad, bd)
    io, inter, union = mr.iou(a, b)
    same(got.iou, io, "iou")
    same(got.inter, inter, "inter")
    same(got.union, union, "union")
    same(got.iou, GOLD[f"iou{k}_iou"], "iou against the reference")
    same(masks.mask_iou(ad != 0, bd != 0), GOLD[f"iou{k}_iou"], "masks.mask_iou against the reference")
    same(masks.masks_to_boxes(ad, list(range(n))), GOLD[f"iou{k}_boxes"].reshape(n, 4), "masks_to_boxes against the reference")
    same_results(geometry.mask_iou(ad, bd), got)
    same_results(geometry.mask_iou(ad != 0, bd != 0), got)
    assert torch.equal(ad.cpu(), torch.from_numpy(a)) and torch.equal(bd.cpu(), torch.from_numpy(b))


def test_iou_clip_axis_other_size_and_special_pairs():
    H, W = mc.SIZES[1]
    a = np.stack([mc.iou_masks(5, H, W, seed=1), mc.iou_masks(5, H, W, seed=2)])        # T = 2
    b = np.stack([mc.iou_masks(3, H, W, seed=3), mc.iou_masks(3, H, W, seed=4)])
    got = geometry.mask_iou(dev(a), dev(b))
    assert tuple(got.iou.shape) == (2, 5, 3)
    for t in range(2):
        for field, want in zip(got, mr.iou(a[t], b[t])):
            same(field[t], want, f"clip {t}")
        same_results(geometry.mask_iou(dev(a[t]), dev(b[t])), [f[t] for f in got])      # a clip alone
    own = geometry.mask_iou(dev(a[0]), dev(a[0]))
    assert float(own.iou[0, 1]) == 1.0 and int(own.inter[0, 3]) == 0 and int(own.union[2, 2]) == 0 and float(own.iou[2, 2]) == 0.0
    assert int(own.inter[4, 4]) == 1
    for h, w in mc.DEGENERATE:
        x = mc.iou_masks(5, h, w, seed=5)
        for field, want in zip(geometry.mask_iou(dev(x), dev(x)), mr.iou(x, x)):
            same(field, want, f"{h} x {w}")


# ---- NMS -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", ["plain", "ties", "nan", "holes", "all"])
@pytest.mark.parametrize("n", mc.NMS_COUNTS)
def test_nms_equals_restatement(n, flavour):
    io, scores, valid = mc.nms_problem(n, seed=300 + n if flavour == "plain" else 400 + n, ties=flavour in ("ties", "all"),
                                       nan=flavour in ("nan", "all"), holes=flavour in ("holes", "all"))
    iod, sd, vd = dev(io), dev(scores), None if valid is None else dev(valid)
    for thr in mc.NMS_THRESHOLDS:
        keep = geometry.nms_greedy(iod, sd, thr, valid=vd)
        same(keep, mr.nms(io, scores, thr, valid), f"keep at {thr}")
        assert torch.equal(keep, geometry.nms_greedy(iod, sd, thr, valid=vd))
        if flavour == "plain":
            kept = masks.generic_nms(iod, sd, thr)
            assert kept.dtype == torch.int64 and host(kept).tolist() == GOLD[f"nms{n}_kept_{thr}"].tolist()
    assert torch.equal(iod.cpu(), torch.from_numpy(io)) and torch.equal(sd.cpu().view(torch.int32), torch.from_numpy(scores).view(torch.int32))


def test_nms_chain_clip_axis_and_nms_masks():
    io, scores = mc.nms_chain()
    assert host(geometry.nms_greedy(dev(io), dev(scores), 0.5)).tolist() == [True, False, True]
    probs = [mc.nms_problem(65, seed=500 + t, ties=True, nan=True, holes=True) for t in range(2)]     # T = 2
    iod, sd, vd = (dev(np.stack([p[k] for p in probs])) for k in range(3))
    keep = geometry.nms_greedy(iod, sd, 0.5, valid=vd)
    assert tuple(keep.shape) == (2, 65)
    for t in range(2):
        same(keep[t], mr.nms(*probs[t][:2], 0.5, probs[t][2]), f"problem {t}")
        assert torch.equal(keep[t], geometry.nms_greedy(iod[t], sd[t], 0.5, valid=vd[t]))
    # nms_masks = generic_nms on the detections above the threshold, scattered back
    H, W = mc.SIZES[0]
    rng = np.random.default_rng(9)
    base = mc.iou_masks(4, H, W, seed=6)
    det = np.concatenate([base, base[[0, 1, 3]], mc.iou_masks(5, H, W, seed=7)])        # duplicates: IoU 1 with their twins
    logits = dev(np.where(det != 0, 2.5, -1.5).astype(np.float32))
    p = dev(rng.random(len(det)).astype(np.float32))
    keep = masks.nms_masks(p, logits, 0.3, 0.5)
    valid = p > 0.3
    idx = torch.nonzero(valid)[:, 0]
    sub = geometry.mask_iou(logits[idx] > 0, logits[idx] > 0).iou
    want = torch.zeros_like(valid)
    want[idx[masks.generic_nms(sub, p[idx], 0.5)]] = True
    assert keep.dtype == torch.bool and torch.equal(keep, want) and bool(keep.any()) and not bool(keep[valid].all())
    same(keep, mr.nms(mr.iou(det, det)[0], host(p), 0.5, host(valid)), "nms_masks against the restatement")


# ---- the reference's names -------------------------------------------------------------------------------------------------
def test_connected_components_edt_and_fill_holes_mirrors():
    H, W = mc.SIZES[0]
    m = mc.batch(mc.rings(H, W))
    labels, counts = masks.connected_components(dev(m)[:, None])
    want = mr.components_batch(m, 8, 0)
    assert tuple(labels.shape) == (mc.B, 1, H, W)
    same(labels[:, 0], want[0], "labels")
    same(counts[:, 0], want[1], "counts")
    assert torch.equal(masks.connected_components(dev(m) != 0)[1], counts[:, 0])
    same(masks.edt(dev(m)), mr.edt_dist(np.stack([mr.edt_d2(k) for k in m])), "edt")
    rng = np.random.default_rng(3)
    scores = np.where(m != 0, 1.0, -1.0).astype(np.float32)
    scores[:, 5:H - 5, 5:W - 5] = 1.0
    scores[rng.random(scores.shape) < 0.02] *= -1.0                 # holes and sprinkles of a few pixels
    sd = dev(scores)[:, None]
    for max_area, kw in ((1, {}), (4, {}), (4, dict(fill_holes=False)), (4, dict(remove_sprinkles=False)), (2000, {})):
        got = masks.fill_holes_in_mask_scores(sd, max_area, **kw)
        want = np.stack([mr.fill_holes(s, max_area, kw.get("fill_holes", True), kw.get("remove_sprinkles", True)) for s in scores])
        same(got[:, 0], want, f"fill_holes {max_area} {kw}")
    assert masks.fill_holes_in_mask_scores(sd, 0) is sd
    assert torch.equal(sd[:, 0].cpu(), torch.from_numpy(scores))


@pytest.mark.parametrize("padding", [True, False])
def test_sample_one_point_from_error_center(padding):
    H, W = mc.SIZES[0]
    rng = np.random.default_rng(4)
    gt = np.zeros((4, H, W), dtype=bool)
    pred = np.zeros((4, H, W), dtype=bool)
    gt[0, 5:30, 10:40] = True                   # prediction empty: a positive click in the middle of gt
    gt[1, 5:15, 5:15] = pred[1, 5:15, 5:15] = True
    pred[1, 20:33, 30:60] = True                # a false positive region: a negative click
    gt[2, 3:12, 3:12] = pred[2, 20:29, 40:49] = True     # equal depths: not strictly larger, so negative
    gt[3], pred[3] = rng.random((H, W)) < 0.6, rng.random((H, W)) < 0.5
    points, labels = masks.sample_one_point_from_error_center(dev(gt)[:, None], dev(pred)[:, None], padding)
    assert tuple(points.shape) == (4, 1, 2) and tuple(labels.shape) == (4, 1)
    want = [mr.error_centre_point(gt[b], pred[b], padding) for b in range(4)]
    assert host(points)[:, 0].tolist() == [list(w[0]) for w in want] and host(labels)[:, 0].tolist() == [w[1] for w in want]
    assert host(labels)[:3, 0].tolist() == [1, 0, 0]
    none = masks.sample_one_point_from_error_center(dev(gt)[:1, None], None, padding)
    assert torch.equal(none[0], points[:1]) and int(none[1]) == 1


def test_person_boxes_feed_process_front_clip():
    H, W = mc.SIZES[0]
    clip = mc.person_clip(2, 2, H, W)
    cd = dev(clip)
    for max_area in (0, 2):
        boxes, area = masks.person_boxes(cd, max_area)
        assert boxes.dtype == torch.float64 and tuple(boxes.shape) == (2, 2, 4) and area.dtype == torch.int32
        for t in range(2):
            for n in range(2):
                cleaned = clip[t, n] if max_area == 0 else mr.fill_holes(np.where(clip[t, n] != 0, 1.0, -1.0), max_area) > 0
                want, wa = mr.largest_component_box(cleaned)
                same(boxes[t, n], want, f"box {t} {n} at max_area {max_area}")
                assert int(area[t, n]) == wa
        assert int(area[0, 0]) == (18 * 11 - 1 if max_area == 0 else 18 * 11) and bool(torch.isnan(boxes[1, 1]).all())
    boxes = masks.person_boxes(cd != 0)[0]
    frames = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    res = bev.process_front_clip(frames, boxes, blank_bev=True)
    foot = bev.foot_from_bbox_xyxy(bev.unnormalize_bbox(bev.convert_xywh_to_xyxy(boxes), (1080, 1920)))
    same(res.foot_uv, host(foot), "foot_uv")
    fm = host(res.foot_m)
    assert np.isfinite(fm[0]).all() and np.isfinite(fm[1, 0]).all() and np.isnan(fm[1, 1]).all()


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_empty_batches_launch_nothing():
    z = torch.zeros((0, 5, 7), dtype=torch.uint8, device="cuda")
    c = geometry.mask_components(z)
    assert tuple(c.labels.shape) == (0, 5, 7) and tuple(c.count.shape) == (0,) and tuple(c.stats.shape) == (0, 256, 7)
    assert tuple(geometry.distance_transform(z).dist.shape) == (0, 5, 7) and tuple(geometry.mask_inner_point(z)[0].shape) == (0, 2)
    assert tuple(geometry.mask_boxes(z).xyxy.shape) == (0, 4)
    assert tuple(geometry.mask_iou(z, torch.zeros((3, 5, 7), dtype=torch.bool, device="cuda")).iou.shape) == (0, 3)
    assert tuple(geometry.nms_greedy(torch.zeros((0, 0), device="cuda"), torch.zeros(0, device="cuda"), 0.5).shape) == (0,)
    assert tuple(masks.masks_to_boxes(z).shape) == (0, 4)


def test_bad_arguments_raise_before_any_launch():
    ok = torch.zeros((2, 5, 7), dtype=torch.uint8, device="cuda")
    calls = [lambda: geometry.mask_components(ok.float()), lambda: geometry.mask_components(ok.cpu()),
             lambda: geometry.mask_components(ok, connectivity=6), lambda: geometry.mask_components(ok, max_components=-1),
             lambda: geometry.mask_components(torch.zeros((2, 0, 7), dtype=torch.uint8, device="cuda")),
             lambda: geometry.mask_components(ok[None, None]), lambda: geometry.distance_transform(ok.to(torch.int32)),
             lambda: geometry.distance_transform(ok.cpu()), lambda: geometry.mask_inner_point(torch.zeros((2, 5, 0), dtype=torch.bool, device="cuda")),
             lambda: geometry.mask_boxes(ok.cpu()), lambda: geometry.mask_boxes(ok.half()),
             lambda: geometry.mask_iou(ok, ok.cpu()), lambda: geometry.mask_iou(ok, ok[:, :4]), lambda: geometry.mask_iou(ok, ok[None]),
             lambda: geometry.nms_greedy(torch.zeros((1025, 1025), device="cuda"), torch.zeros(1025, device="cuda"), 0.5),
             lambda: geometry.nms_greedy(torch.zeros((3, 3)), torch.zeros(3, device="cuda"), 0.5),
             lambda: geometry.nms_greedy(torch.zeros((3, 3), device="cuda"), torch.zeros(4, device="cuda"), 0.5),
             lambda: geometry.nms_greedy(torch.zeros((3, 3), device="cuda"), torch.zeros(3, device="cuda"), 0.5, valid=torch.zeros(3, device="cuda")),
             lambda: geometry.mask_components(torch.zeros((1, 5, 4097), dtype=torch.uint8, device="cuda"))]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
