"""A NumPy restatement of the mask analysis (csrc/masks.hip; rules: include/skimi.h) that shares no code with the kernels:
components by a plain flood fill in raster order, the squared distance transform by brute force over all zero pixels, boxes,
IoU and NMS as straight loops, and the reference's compositions (fill_holes, the error-centre point) on top of them."""
import numpy as np

EDT_NONE = 1 << 30
NEIGHBOURS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
              8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def components(mask, connectivity=8, max_components=256):
    """one mask [H, W] -> labels int32, areas int32, count, stats int64 [max_components, 7]"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    labels = np.zeros((H, W), dtype=np.int32)
    areas = np.zeros((H, W), dtype=np.int32)
    stats = np.zeros((max_components, 7), dtype=np.int64)
    count = 0
    for y0 in range(H):
        for x0 in range(W):
            if not m[y0, x0] or labels[y0, x0]:
                continue
            count += 1
            labels[y0, x0] = count
            stack, pixels = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                for dy, dx in NEIGHBOURS[connectivity]:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and m[v, u] and not labels[v, u]:
                        labels[v, u] = count
                        stack.append((v, u))
            ys, xs = np.array(pixels, dtype=np.int64).T
            areas[ys, xs] = len(pixels)
            if count <= max_components:
                stats[count - 1] = (len(pixels), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum())
    return labels, areas, count, stats


def components_batch(masks, connectivity=8, max_components=256):
    out = [components(m, connectivity, max_components) for m in masks]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int32),
            np.stack([o[3] for o in out]))


def edt_d2(mask, border_zero=False):
    """one mask [H, W] -> int32 [H, W]: the squared distance to the nearest zero pixel, every zero tried"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    zy, zx = np.nonzero(~m)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    best = np.full((H, W), EDT_NONE, dtype=np.int64)
    for k0 in range(0, len(zy), 256):
        dy = ys[..., None] - zy[k0:k0 + 256]
        dx = xs[..., None] - zx[k0:k0 + 256]
        best = np.minimum(best, (dy * dy + dx * dx).min(axis=-1))
    if border_zero:   # the nearest position outside the image is straight across the nearest edge
        for d in (xs + 1, W - xs, ys + 1, H - ys):
            best = np.minimum(best, d * d)
    return best.astype(np.int32)


def edt_dist(d2):
    with np.errstate(all="ignore"):
        dist = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return np.where(d2 >= EDT_NONE, np.float32(np.inf), dist)


def inner_point(mask, border_zero=True):
    """-> ((x, y), d2) of the largest d2, the first in raster order"""
    d2 = edt_d2(mask, border_zero)
    best, at = -1, (0, 0)
    for y in range(d2.shape[0]):
        for x in range(d2.shape[1]):
            if d2[y, x] > best:
                best, at = int(d2[y, x]), (x, y)
    return at, best


def boxes(masks):
    """[N, H, W] -> xyxy int32 [N, 4], area int32 [N]; an empty mask: (W, H, 0, 0)"""
    N, H, W = masks.shape
    xyxy = np.zeros((N, 4), dtype=np.int32)
    area = np.zeros(N, dtype=np.int32)
    for n in range(N):
        x0, y0, x1, y1 = W, H, 0, 0
        for y in range(H):
            for x in range(W):
                if masks[n, y, x]:
                    x0, y0, x1, y1 = min(x0, x), min(y0, y), max(x1, x), max(y1, y)
                    area[n] += 1
        xyxy[n] = (x0, y0, x1, y1)
    return xyxy, area


def iou(a, b):
    """[N, H, W], [M, H, W] -> iou float32, inter, union int32 [N, M]"""
    N, M = a.shape[0], b.shape[0]
    inter = np.zeros((N, M), dtype=np.int32)
    union = np.zeros((N, M), dtype=np.int32)
    for n in range(N):
        for m in range(M):
            inter[n, m] = np.count_nonzero((a[n] != 0) & (b[m] != 0))
            union[n, m] = np.count_nonzero((a[n] != 0) | (b[m] != 0))
    return inter.astype(np.float32) / np.maximum(union, 1).astype(np.float32), inter, union


def nms(iou_matrix, scores, threshold, valid=None):
    """-> keep bool [N]: by score descending, ties (-0 = +0) to the lower index; invalid or NaN entries take no part"""
    N = len(scores)
    s = np.asarray(scores, dtype=np.float32)
    ok = ~np.isnan(s) & (np.ones(N, dtype=bool) if valid is None else np.asarray(valid, dtype=bool))
    order = sorted((i for i in range(N) if ok[i]), key=lambda i: (-float(s[i]), i))
    thr = np.float32(threshold)
    keep = np.zeros(N, dtype=bool)
    dead = np.zeros(N, dtype=bool)
    for k, i in enumerate(order):
        if dead[i]:
            continue
        keep[i] = True
        for j in order[k + 1:]:
            if np.float32(iou_matrix[i, j]) > thr:
                dead[j] = True
    return keep


def fill_holes(scores, max_area, fill=True, sprinkles=True):
    """one score map [H, W] float32 -> the reference's fill_holes_in_mask_scores on it"""
    s = np.array(scores, dtype=np.float32)
    if max_area <= 0:
        return s
    if fill:
        bg = s <= 0
        s = np.where(bg & (components(bg, 8, 0)[1] <= max_area), np.float32(0.1), s)
    if sprinkles:
        fg = s > 0
        thresh = min(int(fg.sum()) // 2, max_area)
        s = np.where(fg & (components(fg, 8, 0)[1] <= thresh), np.float32(-0.1), s)
    return s


def error_centre_point(gt, pred, padding=True):
    """one pair of masks [H, W] -> ((x, y), label)"""
    gt, pred = np.asarray(gt, dtype=bool), np.asarray(pred, dtype=bool)
    fn_at, fn_d2 = inner_point(gt & ~pred, padding)
    fp_at, fp_d2 = inner_point(~gt & pred, padding)
    return (fn_at, 1) if fn_d2 > fp_d2 else (fp_at, 0)


def largest_component_box(mask, max_components=256):
    """one mask -> ((x, y, w, h) / (W, H, W, H) of its largest component, ties to the lowest label; area), NaN when empty"""
    H, W = mask.shape
    _, _, count, stats = components(mask, 8, max_components)
    best = None
    for row in stats[:min(count, max_components)]:
        if best is None or row[0] > best[0]:
            best = row
    if best is None:
        return np.full(4, np.nan), 0
    return np.array([best[1] / W, best[2] / H, (best[3] - best[1]) / W, (best[4] - best[2]) / H], dtype=np.float64), int(best[0])
