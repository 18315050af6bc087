"""CPU: the restatement of the association and tracking rules (tests/assign_restated.py) against scipy's
linear_sum_assignment, against the reference's own associate_det_trk (tests/golden/assign.npz) and against tracks written
out by hand; and the wrappers' argument checks, which need no device."""
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import assign_cases as ac
import assign_restated as ar
from skiing_analysis_pytorch_amd import geometry, masks, tracks

GOLD = np.load(Path(__file__).resolve().parent / "golden" / "assign.npz")


def scipy_solve(c):
    c = np.asarray(c, dtype=np.float64)
    rows, cols = linear_sum_assignment(c)
    total = np.float64(0.0)
    for r, k in zip(rows, cols):                    # ascending rows, one addition each
        total = total + c[r, k]
    return rows, cols, total


# ---- the solver ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", ac.SIZES)
def test_integer_costs_have_a_unique_optimum_and_it_is_scipys(n, m):
    c = ac.costs("integer", n, m, ac.seed_of("integer", n, m))
    assert ac.unique_optimum(c), "a condition on the inputs: pick another seed"
    row_to_col, col_to_row, total, status = ar.solve(c)
    rows, cols, want = scipy_solve(c)
    assert status == 0 and ar.valid_assignment(row_to_col, col_to_row, n, m)
    assert row_to_col[rows].tolist() == cols.tolist()
    assert total == want                            # integers below 2^30: every sum is exact


@pytest.mark.parametrize("kind", ["iou", "equal"])
@pytest.mark.parametrize("n,m", ac.SIZES)
def test_tied_costs_give_a_valid_assignment_with_scipys_total(n, m, kind):
    c = ac.costs(kind, n, m, ac.seed_of(kind, n, m))
    row_to_col, col_to_row, total, status = ar.solve(c)
    assert status == 0 and ar.valid_assignment(row_to_col, col_to_row, n, m)
    # costs O(1), n <= 1024: float64 rounding of the duals is of order n 2^-52
    assert abs(total - scipy_solve(c)[2]) <= 1e-9


def test_non_finite_and_ragged_blocks():
    row_to_col, col_to_row, total, status = ar.solve_batch(ac.nonfinite_costs())
    assert status.tolist() == [1, 0, 1] and np.isnan(total[[0, 2]]).all() and (row_to_col[[0, 2]] == -1).all() and (col_to_row[[0, 2]] == -1).all()
    c, n_rows, n_cols = ac.ragged_batch()
    row_to_col, col_to_row, total, status = ar.solve_batch(c, n_rows, n_cols)
    assert not status.any()
    for b, (r, k) in enumerate(zip(n_rows, n_cols)):
        assert ar.valid_assignment(row_to_col[b], col_to_row[b], r, k)
        assert total[b] == scipy_solve(c[b, :r, :k])[2]
    assert np.array_equal(ar.solve_batch(c, n_rows, n_cols, maximize=True)[2], ar.solve_batch(-c, n_rows, n_cols)[2])


# ---- associate_det_trk against the reference's own results ------------------------------------------------------------------------
def restated_association(name):
    det, trk, scores = ac.assoc_case(name)
    assert str(GOLD[f"{name}_digest"]) == hashlib.sha256(det.tobytes() + trk.tobytes() + scores.tobytes()).hexdigest(), "the golden's inputs"
    iou = ar.mask_iou(det, trk)
    return iou, ar.associate(iou, scores, **ac.ASSOC_THRESHOLDS)


def golden_lists(name):
    """the golden's arrays -> the reference's four objects, scores rounded to float32 (the reference multiplies the float32
    score and IoU as Python floats, which is exact; one rounding to float32 is the float32 product)"""
    N, M = GOLD[f"{name}_det_trk"].shape
    rows = GOLD[f"{name}_scores"].astype(np.float32)
    return ([d for d in range(N) if GOLD[f"{name}_new"][d]], [t for t in range(M) if GOLD[f"{name}_unmatched"][t]],
            {d: [t for t in range(M) if GOLD[f"{name}_det_trk"][d, t]] for d in range(N) if GOLD[f"{name}_det_trk"][d].any()},
            {int(t): [float(rows[t, 0]), float(rows[t, 1])] for t in GOLD[f"{name}_score_order"]})


@pytest.mark.parametrize("name", ac.UNIQUE_CASES)
def test_association_equals_reference_where_the_optimum_is_unique(name):
    iou, res = restated_association(name)
    assert (iou > 0).all() and len(np.unique(iou)) == iou.size, "a condition on the inputs: positive, distinct IoUs"
    assert ac.unique_optimum(np.float32(1) - iou)
    got, want = ar.association_lists(res), golden_lists(name)
    assert got == want
    assert list(got[3]) == list(want[3]), "the order of the score dictionary"


@pytest.mark.parametrize("name", [k for k in ac.ASSOC_CASES if k not in ac.UNIQUE_CASES])
def test_association_tie_invariant_outputs_equal_reference(name):
    iou, res = restated_association(name)
    got, want = ar.association_lists(res), golden_lists(name)
    assert got[0] == want[0] and got[2] == want[2]
    # An assigned pair at zero IoU is a tie (every such pair costs 1) and decides nothing: a track is matched only at iou >=
    # iou_threshold_trk > 0.  The unmatched tracks are compared when no assigned pair above zero sits at a tie: every such
    # pair, of this solution and of scipy's, is part of EVERY optimum (forbidding it raises the total), so both hold the same.
    c = (np.float32(1) - iou).astype(np.float64)
    rows, cols, best = scipy_solve(c)
    pairs = {(int(r), int(k)) for r, k in zip(rows, cols)} | {(int(d), t) for t, d in enumerate(res["trk_to_det"]) if d >= 0}

    def forced(r, k):
        d = c.copy()
        d[r, k] = 1e18
        rr, kk = linear_sum_assignment(d)
        return d[rr, kk].sum() > best + 1e-9

    assert all(forced(r, k) for r, k in pairs if iou[r, k] > 0), "a condition on the inputs: pick another seed"
    assert got[1] == want[1]


# ---- the tracker -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ac.link_clips()))
def test_tracker_on_hand_built_clips(name):
    boxes, scores, params, want_ids, (want_tracks, want_overflow) = ac.link_clips()[name]
    ids, n_tracks, table, overflow = ar.link_boxes(boxes, scores, **params)
    assert ids.tolist() == want_ids.tolist()
    assert (n_tracks, overflow) == (want_tracks, want_overflow)
    for k in range(n_tracks):
        frames = np.argwhere((ids == k).any(axis=1))[:, 0]
        assert table[k].tolist() == [frames[0], frames[-1], len(frames)]
    assert (table[n_tracks:] == [-1, -1, 0]).all()


def test_tracker_written_out():
    """the ids of the crossing, the gaps and the overflow, as numbers"""
    clips = ac.link_clips()
    assert ar.link_boxes(clips["cross"][0], None, **clips["cross"][2])[0].tolist() == [[0, 1]] * 6 + [[1, 0]] * 6
    assert ar.link_boxes(clips["gap_max_age"][0], None, **clips["gap_max_age"][2])[0][:, 0].tolist() == [0, 0, -1, -1, -1, 0, 0]
    assert ar.link_boxes(clips["gap_longer"][0], None, **clips["gap_longer"][2])[0][:, 0].tolist() == [0, 0, -1, -1, -1, -1, 1, 1]
    assert ar.link_boxes(clips["empty_frame"][0], None, **clips["empty_frame"][2])[0].tolist() == [[0, 1], [-1, -1], [0, 1]]
    ids, n, _, overflow = ar.link_boxes(clips["overflow"][0], None, **clips["overflow"][2])
    assert ids.tolist() == [[0, 1, -1], [-1, 0, -1]] and (n, overflow) == (2, 3)
    assert ar.link_boxes(*clips["nan_and_scores"][:2], **clips["nan_and_scores"][2])[0].tolist() == [[0, -1, -1], [0, 1, 2], [0, 1, 2]]


def test_track_helpers_on_the_host():
    """track_boxes, main_track and the lists helper are plain torch ops: they run wherever their inputs are"""
    ids = torch.tensor([[1, 0, -1], [-1, 1, 2], [0, -1, -1]], dtype=torch.int32)
    boxes = torch.arange(36, dtype=torch.float64).reshape(3, 3, 4)
    per = tracks.track_boxes(ids, boxes, 3)
    assert tuple(per.shape) == (3, 3, 4)
    assert torch.equal(per[0, 0], boxes[0, 1]) and torch.equal(per[0, 1], boxes[0, 0]) and torch.isnan(per[0, 2]).all()
    assert torch.isnan(per[1, 0]).all() and torch.equal(per[1, 1], boxes[1, 1]) and torch.equal(per[1, 2], boxes[1, 2])
    assert torch.equal(tracks.track_boxes(ids, boxes, 2).nan_to_num(nan=-1.0), per[:, :2].nan_to_num(nan=-1.0))   # the id past K is cut off
    table = torch.tensor([[0, 2, 2], [0, 1, 2], [1, 1, 1]], dtype=torch.int32)
    assert int(tracks.main_track(table)) == 0 and int(tracks.main_track(table.flip(0))) == 1
    assert tracks.main_track(table[None].expand(2, 3, 3)).tolist() == [0, 0]
    assert masks.association_lists(masks.Association(torch.zeros(0, dtype=torch.int32), None, None, torch.zeros(3, dtype=torch.bool),
                                                     None, None)) == ([0, 1, 2], [], {}, {})


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    from skiing_analysis_pytorch_amd import _lib

    lib = _lib.lib()
    assert lib.skimi_linear_assignment(None, None, None, 1, 3, 3, None, None, None, None, None) != 0 and b"NULL" in lib.skimi_last_error()
    assert lib.skimi_linear_assignment(None, None, None, 1, 1025, 3, None, None, None, None, None) != 0 and b"1024" in lib.skimi_last_error()
    assert lib.skimi_linear_assignment(None, None, None, 0, 3, 3, None, None, None, None, None) != 0
    assert lib.skimi_link_boxes(None, None, 1, 4, 2, 4, 0.3, 15, 0.0, None, None, None, None, None) != 0 and b"NULL" in lib.skimi_last_error()
    assert lib.skimi_link_boxes(None, None, 1, 4, 65, 4, 0.3, 15, 0.0, None, None, None, None, None) != 0 and b"64" in lib.skimi_last_error()
    assert lib.skimi_link_boxes(None, None, 1, 4, 2, 4, 0.3, -1, 0.0, None, None, None, None, None) != 0 and b"max_age" in lib.skimi_last_error()
    assert lib.skimi_link_boxes(None, None, 1, 4, 2, 4, float("nan"), 15, 0.0, None, None, None, None, None) != 0



def test_wrappers_reject_host_tensors_dtypes_and_sizes():
    assert geometry.ASSIGN_MAX == geometry.NMS_MAX == 1024 and geometry.LINK_MAX == 64
    with pytest.raises(ValueError, match="device tensor"):
        geometry.linear_assignment(torch.zeros(2, 3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32 or float64"):
        geometry.linear_assignment(torch.zeros(2, 3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="float32 or float64"):
        geometry.linear_assignment(np.zeros((3, 4)))
    with pytest.raises(ValueError, match="at most 1024"):
        geometry.linear_assignment(torch.zeros(1, geometry.ASSIGN_MAX + 1, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="at most 1024"):
        geometry.linear_assignment(torch.zeros(2, geometry.ASSIGN_MAX + 1, dtype=torch.float32))
    with pytest.raises(ValueError, match=r"\[N, M\] or \[B, N, M\]"):
        geometry.linear_assignment(torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="device tensor"):
        geometry.link_boxes(torch.zeros(5, 2, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        geometry.link_boxes(torch.zeros(5, 2, 4, dtype=torch.float32))
    with pytest.raises(ValueError, match="at most 64"):
        geometry.link_boxes(torch.zeros(5, 65, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="at most 64"):
        geometry.link_boxes(torch.zeros(5, 2, 4, dtype=torch.float64), max_tracks=0)
    with pytest.raises(ValueError, match=r"\[T, N, 4\]"):
        geometry.link_boxes(torch.zeros(5, 2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="max_age"):
        geometry.link_boxes(torch.zeros(5, 2, 4, dtype=torch.float64), max_age=-1)
    with pytest.raises(ValueError, match="det_scores is required"):
        masks.associate_det_trk(torch.zeros(2, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="one size"):
        masks.associate_det_trk(torch.zeros(2, 4, 4), torch.zeros(3, 4, 5), det_scores=torch.zeros(2))
    with pytest.raises(ValueError, match="device tensor"):
        masks.associate_det_trk(torch.zeros(2, 4, 4, dtype=torch.bool), torch.zeros(3, 4, 4, dtype=torch.bool), det_scores=torch.zeros(2))
