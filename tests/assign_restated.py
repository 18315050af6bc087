"""NumPy restatement of the association and tracking rules of include/skimi.h (csrc/assign.hip, csrc/lsap.h, the package's
masks.associate_det_trk and tracks.py): what the kernels compute, operation for operation in float64, so that the device
results can be compared bit for bit.  Nothing here is fast."""
import numpy as np

INF = np.inf


def solve(cost):
    """One problem, cost [n, m] -> (row_to_col int32 [n], col_to_row int32 [m], total float64, status int32).  Rules 1 - 5 of
    skimi_linear_assignment."""
    c = np.asarray(cost).astype(np.float64)
    n, m = c.shape
    row_to_col, col_to_row = np.full(n, -1, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    failed = (row_to_col, col_to_row, np.float64(np.nan), np.int32(1))
    if not np.isfinite(c).all():
        return failed
    tr = n > m
    a = c.T if tr else c
    nr, nc = a.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    with np.errstate(over="ignore", invalid="ignore"):
        for cur in range(nr):
            sp, pred, seen = np.full(nc, INF), np.full(nc, -1), np.zeros(nc, dtype=bool)
            minv, i, sink = np.float64(0.0), cur, -1
            while sink < 0:
                r = ((minv + a[i]) - u[i]) - v
                better = ~seen & (r < sp)
                sp[better], pred[better] = r[better], i
                cand = np.where(seen, INF, sp)
                j = int(np.argmin(cand))            # the first of the smallest: ties to the lowest column
                if not cand[j] < INF:
                    return failed
                minv, seen[j] = cand[j], True
                if row4col[j] < 0:
                    sink = j
                else:
                    i = row4col[j]
            upd = seen.copy()
            upd[sink] = False
            d = minv - sp[upd]
            u[row4col[upd]] = u[row4col[upd]] + d   # the rows of distinct assigned columns are distinct
            v[upd] = v[upd] - d
            u[cur] = u[cur] + minv
            j = sink
            while True:
                i = pred[j]
                row4col[j] = i
                col4row[i], j = j, col4row[i]
                if i == cur:
                    break
    if tr:
        row_to_col[:], col_to_row[:] = row4col, col4row
    else:
        row_to_col[:], col_to_row[:] = col4row, row4col
    total = np.float64(0.0)
    for i in range(n):
        if row_to_col[i] >= 0:
            total = total + c[i, row_to_col[i]]
    return row_to_col, col_to_row, total, np.int32(0)


def solve_batch(cost, n_rows=None, n_cols=None, maximize=False):
    """cost [B, N, M] -> row_to_col int32 [B, N], col_to_row int32 [B, M], total float64 [B], status int32 [B]"""
    c = np.asarray(cost).astype(np.float64)
    c = -c if maximize else c
    B, N, M = c.shape
    r2c, c2r = np.full((B, N), -1, dtype=np.int32), np.full((B, M), -1, dtype=np.int32)
    total, status = np.zeros(B), np.zeros(B, dtype=np.int32)
    for b in range(B):
        nr = N if n_rows is None else int(n_rows[b])
        nc = M if n_cols is None else int(n_cols[b])
        r2c[b, :nr], c2r[b, :nc], total[b], status[b] = solve(c[b, :nr, :nc])
    return r2c, c2r, total, status


def valid_assignment(row_to_col, col_to_row, n, m):
    """the maps are inverse to each other and hold min(n, m) pairs inside the block"""
    rows = [i for i in range(len(row_to_col)) if row_to_col[i] >= 0]
    cols = [j for j in range(len(col_to_row)) if col_to_row[j] >= 0]
    return (len(rows) == len(cols) == min(n, m) and all(i < n and 0 <= row_to_col[i] < m and col_to_row[row_to_col[i]] == i for i in rows)
            and all(row_to_col[col_to_row[j]] == j for j in cols))


# ---- associate_det_trk -----------------------------------------------------------------------------------------------------------
def mask_iou(a, b):
    """a [N, H, W], b [M, H, W] non-zero = foreground -> float32 [N, M] = float32(inter) / float32(max(union, 1))"""
    fa, fb = (a != 0).reshape(len(a), -1), (b != 0).reshape(len(b), -1)
    inter = (fa[:, None, :] & fb[None, :, :]).sum(-1)
    union = (fa[:, None, :] | fb[None, :, :]).sum(-1)
    return inter.astype(np.float32) / np.maximum(union, 1).astype(np.float32)


def associate(iou, scores, iou_threshold=0.5, iou_threshold_trk=0.5, new_det_thresh=0.0, n_det=None, n_trk=None, trk_nonempty=None):
    """One frame: iou float32 [N, M], scores float32 [N] -> the fields of masks.Association as arrays.  Thresholds are
    compared in float32, as torch compares a float32 tensor with a Python number."""
    iou = np.asarray(iou, dtype=np.float32)
    N, M = iou.shape
    nd, nt = N if n_det is None else int(n_det), M if n_trk is None else int(n_trk)
    scores = np.asarray(scores, dtype=np.float32)
    cost = np.float32(1) - iou
    trk_to_det = np.full(M, -1, dtype=np.int32)
    trk_to_det[:nt] = solve(cost[:nd, :nt])[1]
    assigned = trk_to_det >= 0
    at = np.maximum(trk_to_det, 0)
    pair_iou = iou[at, np.arange(M)] if N else np.zeros(M, dtype=np.float32)
    pair_score = scores[at] if N else np.zeros(M, dtype=np.float32)
    trk_ok, det_ok = np.arange(M) < nt, np.arange(N) < nd
    trk_matched = assigned & (pair_iou >= np.float32(iou_threshold_trk))
    trk_unmatched = trk_ok & ~trk_matched
    if trk_nonempty is not None:
        trk_unmatched &= np.asarray(trk_nonempty, dtype=bool)
    det_trk = (iou >= np.float32(iou_threshold)) & det_ok[:, None] & trk_ok[None, :]
    det_new = det_ok & ((~det_trk.any(axis=1) & (scores >= np.float32(new_det_thresh))) | (nt == 0))
    both = np.stack([pair_score, pair_score * pair_iou], axis=-1).astype(np.float32)
    trk_det_scores = np.where(assigned[:, None], both, np.float32(np.nan)).astype(np.float32)
    return dict(trk_to_det=trk_to_det, trk_matched=trk_matched, trk_unmatched=trk_unmatched, det_new=det_new, det_trk=det_trk,
                trk_det_scores=trk_det_scores)


def association_lists(res):
    """associate's dictionary -> the reference's four objects (masks.association_lists' rule)"""
    N, M = res["det_trk"].shape
    if N == 0 or M == 0:
        return list(range(N)), [], {}, {}
    t2d = res["trk_to_det"]
    scores = {t: [float(res["trk_det_scores"][t, 0]), float(res["trk_det_scores"][t, 1])]
              for t in sorted((t for t in range(M) if t2d[t] >= 0), key=lambda t: t2d[t])}
    return ([d for d in range(N) if res["det_new"][d]], [t for t in range(M) if res["trk_unmatched"][t]],
            {d: [t for t in range(M) if res["det_trk"][d, t]] for d in range(N) if res["det_trk"][d].any()}, scores)


# ---- link_boxes ------------------------------------------------------------------------------------------------------------------
def box_iou(a, b):
    """rule 2 of skimi_link_boxes, in its order of operations"""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    inter = iw * ih if iw > 0.0 and ih > 0.0 else np.float64(0.0)
    uni = ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
    return inter / uni if uni > 0.0 else np.float64(0.0)


def link_boxes(boxes, scores=None, iou_threshold=0.3, max_age=15, new_score=0.0, max_tracks=64):
    """One clip: boxes float64 [T, N, 4], scores [T, N] or None -> ids int32 [T, N], n_tracks, table int32 [K, 3], overflow"""
    boxes = np.asarray(boxes, dtype=np.float64)
    T, N = boxes.shape[:2]
    K = int(max_tracks)
    ids = np.full((T, N), -1, dtype=np.int32)
    table = np.tile(np.array([-1, -1, 0], dtype=np.int32), (K, 1))
    last_box, age = [], []
    overflow = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T):
            dets = [d for d in range(N) if np.isfinite(boxes[t, d]).all()]
            live = [k for k in range(len(last_box)) if age[k] <= max_age]
            hit = [False] * len(last_box)
            taken = {}
            if dets and live:
                cost = np.array([[np.float64(1.0) - box_iou(boxes[t, d], last_box[k]) for k in live] for d in dets])
                row_to_col, _, _, status = solve(cost)
                if status == 0:
                    for r, d in enumerate(dets):
                        if row_to_col[r] >= 0 and box_iou(boxes[t, d], last_box[live[row_to_col[r]]]) >= iou_threshold:
                            taken[d] = live[row_to_col[r]]
            for d, k in taken.items():
                ids[t, d], last_box[k], hit[k] = k, boxes[t, d].copy(), True
                table[k, 1], table[k, 2] = t, table[k, 2] + 1
            for d in dets:
                if d in taken or not (scores is None or scores[t, d] >= new_score):
                    continue
                if len(last_box) < K:
                    ids[t, d] = len(last_box)
                    table[len(last_box)] = [t, t, 1]
                    last_box.append(boxes[t, d].copy()), age.append(0), hit.append(True)
                else:
                    overflow += 1
            age = [0 if hit[k] else age[k] + 1 for k in range(len(last_box))]
    return ids, np.int32(len(last_box)), table, np.int32(overflow)
