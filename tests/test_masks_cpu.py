"""CPU: the restatement of the mask analysis (tests/masks_restated.py) against independent implementations, so that the GPU
tests compare the kernels with something that is itself pinned: scipy.ndimage for components (labels equal, not merely up to
renaming) and the distance transform, the reference's own masks_to_boxes, mask_iou and generic_nms_cpu (tests/golden/
masks.npz, tools/make_goldens.py's gen_masks), and the record arithmetic of masks.person_boxes on CPU tensors."""
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy import ndimage

import masks_cases as mc
import masks_restated as mr
from skiing_analysis_pytorch_amd import geometry, masks

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "masks.npz")
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), dtype=bool)}
ALL_SIZES = mc.SIZES + mc.DEGENERATE


def test_the_public_names_exist():
    for name in ("mask_components", "distance_transform", "mask_inner_point", "mask_boxes", "mask_iou", "nms_greedy", "ComponentsResult",
                 "EdtResult", "MaskBoxes", "MaskIoU", "EDT_NONE", "NMS_MAX"):
        assert hasattr(geometry, name), name
    assert geometry.EDT_NONE == mr.EDT_NONE == 1 << 30 and geometry.NMS_MAX == 1024


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", ALL_SIZES)
def test_components_equal_scipy_label(size, connectivity):
    for name, m in mc.component_cases(*size).items():
        labels, areas, count, stats = mr.components(m, connectivity, 16)
        want, n = ndimage.label(m, structure=STRUCTURE[connectivity])
        assert count == n, name
        assert np.array_equal(labels, want), name
        sizes = np.bincount(want.ravel(), minlength=n + 1)
        assert np.array_equal(areas, np.where(want > 0, sizes[want], 0)), name
        for k, sl in enumerate(ndimage.find_objects(want)[:16]):
            ys, xs = np.nonzero(want == k + 1)
            assert stats[k].tolist() == [sizes[k + 1], sl[1].start, sl[0].start, sl[1].stop - 1, sl[0].stop - 1, xs.sum(), ys.sum()], name
        assert not stats[n:].any(), name


def test_component_cases_are_what_they_say():
    H, W = mc.SIZES[1]
    c = mc.component_cases(H, W)
    count = {(name, k): mr.components(c[name], k, 0)[2] for name in ("checkerboard", "serpentine", "comb", "u", "rings", "many") for k in (4, 8)}
    assert count["checkerboard", 8] == 1 and count["checkerboard", 4] == (H * W + 1) // 2
    assert count["serpentine", 4] == count["serpentine", 8] == 1 and count["u", 4] == 1 and count["comb", 4] == 1
    assert count["rings", 8] == 3 and count["many", 8] > mc.MANY_MAX_COMPONENTS


@pytest.mark.parametrize("size", ALL_SIZES)
def test_distance_transform_equals_scipy(size):
    cases = dict(mc.edt_cases(*size))
    cases["two_maxima"] = (mc.two_maxima(*mc.SIZES[0]), False)
    seen = 0
    for name, (m, border) in cases.items():
        d2 = mr.edt_d2(m, border)
        assert d2.dtype == np.int32 and (d2[m == 0] == 0).all(), name
        padded = np.pad(m, 1) if border else m
        if not (padded == 0).any():
            assert (d2 == mr.EDT_NONE).all() and np.isinf(mr.edt_dist(d2)).all(), name
            continue
        want = np.rint(ndimage.distance_transform_edt(padded) ** 2).astype(np.int64)
        want = want[1:-1, 1:-1] if border else want
        assert np.array_equal(d2, want), name
        assert np.array_equal(mr.edt_dist(d2), np.sqrt(want.astype(np.float64)).astype(np.float32)), name
        seen += 1
    assert seen >= 8


def test_inner_point_takes_the_first_of_equal_maxima():
    m = mc.two_maxima(*mc.SIZES[0])
    d2 = mr.edt_d2(m, True)
    assert (d2 == d2.max()).sum() >= 2
    (x, y), best = mr.inner_point(m, True)
    assert (x, y) == (43, 13) and best == 16 == d2.max()          # the centre of the upper square, not of the lower one
    assert mr.inner_point(np.zeros((5, 7), dtype=np.uint8)) == ((0, 0), 0)


def test_boxes_and_iou_equal_the_reference():
    for k, (n, m) in enumerate(mc.IOU_SHAPES):
        a, b = GOLD[f"iou{k}_a"], GOLD[f"iou{k}_b"]
        H, W = mc.SIZES[0]
        assert np.array_equal(a, mc.iou_masks(n, H, W, seed=100 + k)) and np.array_equal(b, mc.iou_masks(m, H, W, seed=200 + k))
        io, inter, union = mr.iou(a, b)
        assert io.dtype == np.float32 and np.array_equal(io, GOLD[f"iou{k}_iou"])
        xyxy, area = mr.boxes(a)
        assert np.array_equal(xyxy.astype(np.float32), GOLD[f"iou{k}_boxes"].reshape(n, 4))
        assert np.array_equal(area, (a != 0).sum(axis=(1, 2)))
    assert mr.boxes(np.zeros((1, 4, 9), dtype=np.uint8))[0].tolist() == [[9, 4, 0, 0]]
    a = mc.iou_masks(5, *mc.SIZES[0], seed=100)
    io, inter, union = mr.iou(a, a)
    assert io[0, 1] == 1 and inter[0, 3] == 0 and io[2, 2] == 0 and union[2, 2] == 0      # identical, disjoint, empty


@pytest.mark.parametrize("n", mc.NMS_COUNTS)
def test_nms_equals_the_reference_cpu_loop(n):
    io, scores, _ = mc.nms_problem(n, seed=300 + n)
    assert hashlib.sha256(io.tobytes() + scores.tobytes()).hexdigest() == str(GOLD[f"nms{n}_digest"])
    for thr in mc.NMS_THRESHOLDS:
        keep = mr.nms(io, scores, thr)
        kept = GOLD[f"nms{n}_kept_{thr}"]
        assert sorted(np.nonzero(keep)[0].tolist()) == sorted(kept.tolist())
        assert (np.diff(scores[kept]) < 0).all()


def test_nms_rules():
    io, scores = mc.nms_chain()
    assert mr.nms(io, scores, 0.5).tolist() == [True, False, True]
    assert mr.nms(io, scores, 0.5, valid=[False, True, True]).tolist() == [False, True, False]
    tie = np.array([0.5, -0.0, 0.5, 0.0, np.nan], dtype=np.float32)
    full = np.ones((5, 5), dtype=np.float32)
    assert mr.nms(full, tie, 0.5).tolist() == [True, False, False, False, False]
    assert mr.nms(full, tie, 1.0).tolist() == [True, True, True, True, False]
    assert mr.nms(full, tie, 0.5, valid=[False, True, False, True, True]).tolist() == [False, True, False, False, False]


def test_fill_holes_on_the_nested_rings():
    H, W = mc.SIZES[0]
    m = mc.rings(H, W)
    scores = np.where(m != 0, 1.0, -1.0).astype(np.float32)
    dot = np.zeros((H, W), dtype=bool)
    dot[H // 2, W // 2] = True
    # as drawn, the dot is a one-pixel sprinkle: it goes, both rings stay, and no background component is that small
    out = mr.fill_holes(scores, 1)
    assert out[H // 2, W // 2] == np.float32(-0.1) and np.array_equal(out[~dot], scores[~dot])
    # with the inner ring filled in around it, the dot is a one-pixel hole: it is filled, and the outer ring, the gap between
    # the rings and the outside (all larger than max_area) are left alone
    solid = scores.copy()
    solid[5:H - 5, 5:W - 5] = 1.0
    solid[dot] = -1.0
    out = mr.fill_holes(solid, 1)
    assert out[H // 2, W // 2] == np.float32(0.1) and np.array_equal(out[~dot], solid[~dot])
    assert (out[1, 1:W - 1] == 1.0).all() and out[0, 0] == -1.0 and out[2, 2] == -1.0
    assert np.array_equal(mr.fill_holes(solid, 1, fill=False), solid) and np.array_equal(mr.fill_holes(solid, 0), solid)


def test_person_boxes_record_arithmetic_on_cpu_tensors():
    stats = torch.zeros((2, 3, 4, 7), dtype=torch.int64)
    stats[0, 0, 0] = torch.tensor([5, 2, 3, 6, 4, 0, 0])
    stats[0, 0, 1] = torch.tensor([9, 10, 20, 12, 22, 0, 0])
    stats[0, 0, 2] = torch.tensor([9, 30, 40, 30, 40, 0, 0])     # a tie: the lower label wins
    stats[1, 2, 0] = torch.tensor([1, 7, 8, 7, 8, 7, 8])
    box, area = masks.largest_component_boxes(stats, 100, 50)
    assert box.dtype == torch.float64 and area.dtype == torch.int32 and tuple(box.shape) == (2, 3, 4)
    assert box[0, 0].tolist() == [10 / 100, 20 / 50, 2 / 100, 2 / 50] and area[0, 0] == 9
    assert box[1, 2].tolist() == [7 / 100, 8 / 50, 0.0, 0.0] and area[1, 2] == 1
    assert torch.isnan(box[0, 1]).all() and area[0, 1] == 0
    clip = mc.person_clip(2, 2, *mc.SIZES[0])
    for t in range(2):
        for n in range(2):
            _, _, _, st = mr.components(clip[t, n], 8, 256)
            b, a = masks.largest_component_boxes(torch.from_numpy(st), mc.SIZES[0][1], mc.SIZES[0][0])
            want, wa = mr.largest_component_box(clip[t, n])
            assert np.array_equal(b.numpy(), want, equal_nan=True) and int(a) == wa


def test_bad_arguments_are_value_errors_on_the_host():
    with pytest.raises(ValueError):
        geometry.mask_components(torch.zeros((1, 4, 4), dtype=torch.uint8))       # a host tensor
    with pytest.raises(ValueError):
        geometry.nms_greedy(torch.zeros((2, 2)), torch.zeros(2), 0.5)
