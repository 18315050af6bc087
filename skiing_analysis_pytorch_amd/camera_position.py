"""Counterpart of triangulation/camera_position/camera_position.py's keypoint and ORB paths with the reference's signatures:

    estimate_camera_pose_from_kpt(pts1, pts2, K, baseline_m) -> (R, T (3, 1), mask_pose)        (camera_position.py:88-117)
    estimate_camera_pose_from_ORB(img1, img2, K, baseline_m, max_matches=1000) -> (R, T (3, 1), pose_mask)     (:181-226)

cv2.findEssentialMat(RANSAC, prob 0.999, threshold 1.0) + cv2.recoverPose there; geometry.essential_ransac on the device
here (DESIGN §2 "Essential matrix": 1024 five-point hypotheses, all scored, no early termination).  The reference's callers
(triangulation/view_process/two_view.py, triangulation/estimate_camera_position.py) loop over the frames and call it once
per frame on the 17 keypoints; `estimate_camera_poses_from_kpts` takes all frames as per-frame groups of one call.  The ORB
path (cv2.ORB_create(3000) + cv2.BFMatcher(NORM_HAMMING, crossCheck=True) there) is geometry.orb_features and
geometry.match_hamming here, the project's own detector and descriptor and not OpenCV's (DESIGN §2 "Image features");
`estimate_camera_poses_from_ORB` takes two clips and reads nothing back before the result.  The SIFT paths

    estimate_camera_pose_from_SIFT(img1, img2, K, baseline_m, ratio_thresh=0.75) -> (R, T (3, 1), pts1, pts2, mask_pose)   (:120-178)
    estimate_pose_from_bbox_region(imgL, imgR, bboxL, bboxR, K, baseline_m) -> (R, T (3, 1), mask_pose)                    (:242-297)

(cv2.SIFT_create + BFMatcher.knnMatch(k=2) + Lowe's ratio test there) are geometry.sift_features and geometry.match_l2 here,
again the project's own rules and not OpenCV's (DESIGN §2 "Image features (SIFT-style)"); `estimate_camera_poses_from_SIFT`
takes two clips.  Left out: estimate_pose_from_bbox_and_kpt, whose weighting by repetition needs groups of variable size."""
from __future__ import annotations

import numpy as np
import torch

from . import geometry


def _run(pts1, pts2, K, baseline_m, group_size, hypotheses, seed, group_offset=0):
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dev, torch.float64)   # noqa: E731
    x2d = torch.stack([up(pts1).reshape(-1, 2), up(pts2).reshape(-1, 2)])
    K = up(K).reshape(3, 3)
    return geometry.essential_ransac(x2d, torch.stack([K, K]), group_size=group_size, hypotheses=hypotheses, seed=seed,
                                     group_offset=group_offset, baseline=float(baseline_m))


def estimate_camera_pose_from_kpt(pts1, pts2, K, baseline_m, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0):
    """pts1 (N, 2) the left view's keypoints, pts2 (N, 2) the right view's, K (3, 3) shared, host arrays or tensors ->
    (R (3, 3), T (3, 1), mask_pose (N,) uint8) as host arrays with X2 = R X1 + T and ||-R^T T|| = baseline_m, or three None
    when no essential matrix is found (fewer than 5 usable pairs, none at all included).  mask_pose marks the inliers in
    front of both cameras (cv2's is (N, 1) and votes with outliers too: DESIGN).  group_offset = f draws the samples of
    frame f of estimate_camera_poses_from_kpts."""
    if len(pts1) < 5:
        return None, None, None
    r = _run(pts1, pts2, K, baseline_m, None, hypotheses, seed, group_offset)
    if not bool(r.success[0]):
        return None, None, None
    return r.R[0].cpu().numpy(), r.t[0].cpu().numpy().reshape(3, 1), r.pose_mask.cpu().numpy()


def estimate_camera_poses_from_kpts(pts1, pts2, K, baseline_m, hypotheses: int = 1024, seed: int = 0):
    """Every frame of a clip in one call: pts1, pts2 (T, J, 2) -> (R (T, 3, 3), T (T, 3, 1), mask_pose (T, J) uint8, success
    (T,) bool) as host arrays; a frame without a pose has NaN in R and T.  Frame f is bitwise what
    estimate_camera_pose_from_kpt gives for it with the same seed and group_offset = f."""
    T_, J = np.shape(pts1)[0], np.shape(pts1)[1]
    r = _run(pts1, pts2, K, baseline_m, J, hypotheses, seed)
    ok = r.success.cpu().numpy()
    return r.R.cpu().numpy(), r.t.cpu().numpy().reshape(T_, 3, 1), r.pose_mask.cpu().numpy().reshape(T_, J), ok


def _bgr_u8(img, dev):
    """to_gray_cv_image's inputs, a frame or a clip of them: float in [0, 1] or uint8, [..., H, W, 3] in R, G, B order (or
    [..., H, W] gray), host array or tensor -> uint8 device frames [..., H, W, ch] in B, G, R order"""
    t = (img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))).to(dev)
    if t.is_floating_point():
        t = t.clamp(0, 1).mul(255).to(torch.uint8)      # the reference's .byte(): truncation
    elif t.dtype != torch.uint8:
        raise TypeError(f"frames must be floating point in [0, 1] or uint8, got {t.dtype}")
    if t.shape[-1] != 3:
        return t[..., None].contiguous()
    return t.flip(-1).contiguous()


def _one(im):
    """a frame, host array or tensor -> a clip of that frame"""
    return (im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im)))[None]


def _poses_from_matches(xy1, xy2, pairs, K, baseline_m, hypotheses, seed, group_offset):
    """keypoints xy1, xy2 [T, M, 2] and a matcher's pairs [T, max_matches, 2] (-1 behind the last) -> (essential_ransac's
    result with a group per frame, x2d [2, T, max_matches, 2] NaN-padded) on the device, no read-back"""
    valid = (pairs[..., 0] >= 0)[..., None]
    idx = pairs.clamp(min=0).long()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=pairs.device)
    pick = lambda xy, col: torch.where(valid, torch.gather(xy, 1, idx[..., col, None].expand(-1, -1, 2)), nan)   # noqa: E731
    x2d = torch.stack([pick(xy1, 0), pick(xy2, 1)])
    Kd = (K if isinstance(K, torch.Tensor) else torch.from_numpy(np.asarray(K))).to(pairs.device, torch.float64).reshape(3, 3)
    r = geometry.essential_ransac(x2d.reshape(2, -1, 2), torch.stack([Kd, Kd]), group_size=int(pairs.shape[1]), hypotheses=hypotheses,
                                  seed=seed, group_offset=group_offset, baseline=float(baseline_m))
    return r, x2d


def estimate_camera_poses_from_ORB(frames1, frames2, K, baseline_m, max_matches: int = 1000, max_features: int = 3000,
                                   levels: int = 8, threshold: int = 20, hypotheses: int = 1024, seed: int = 0,
                                   group_offset: int = 0):
    """Every frame pair of two clips in one pass on the device: frames1, frames2 (T, H, W, 3) RGB (float in [0, 1] or
    uint8; or (T, H, W) gray), K (3, 3) shared -> (R (T, 3, 3), T (T, 3, 1), pose_mask (T, max_matches) uint8, success (T,)
    bool) as host arrays.  Features of both clips, cross-checked Hamming matches by (distance, query), the first
    max_matches of them gathered into NaN-padded correspondences, one essential_ransac with a group per frame; pose_mask
    marks the matches (in that order) that are inliers in front of both cameras.  A frame without a pose has NaN in R and T.
    Frame f is bitwise what estimate_camera_pose_from_ORB gives for it with the same seed and group_offset = f."""
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _bgr_u8(frames1, dev), _bgr_u8(frames2, dev)
    if a.dim() != 4 or b.dim() != 4 or a.shape[0] != b.shape[0]:
        raise ValueError(f"estimate_camera_poses_from_ORB: need two clips of T frames, got {list(a.shape)}, {list(b.shape)}")
    T_, mm = int(a.shape[0]), int(max_matches)
    fa = geometry.orb_features(a, max_features, levels, threshold)
    fb = geometry.orb_features(b, max_features, levels, threshold)
    m = geometry.match_hamming(fa.desc, fa.count, fb.desc, fb.count, cross_check=True, max_matches=mm)
    r, _ = _poses_from_matches(fa.xy, fb.xy, m.pairs, K, baseline_m, hypotheses, seed, group_offset)
    return (r.R.cpu().numpy(), r.t.cpu().numpy().reshape(T_, 3, 1), r.pose_mask.cpu().numpy().reshape(T_, mm),
            r.success.cpu().numpy())


def estimate_camera_pose_from_ORB(img1, img2, K, baseline_m, max_matches: int = 1000, max_features: int = 3000, levels: int = 8,
                                  threshold: int = 20, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0):
    """img1, img2 (H, W, 3) RGB, float in [0, 1] or uint8 (the reference's to_gray_cv_image inputs; (H, W) gray too), K
    (3, 3) -> (R (3, 3), T (3, 1), pose_mask (max_matches,) uint8) as host arrays with X2 = R X1 + T and ||T|| = baseline_m,
    or three None when no essential matrix is found (fewer than 5 matches).  pose_mask marks the matches, ordered by
    (distance, query), that are inliers in front of both cameras.  group_offset = f draws the samples of frame f of
    estimate_camera_poses_from_ORB."""
    R, T, mask, ok = estimate_camera_poses_from_ORB(_one(img1), _one(img2), K, baseline_m, max_matches, max_features, levels, threshold,
                                                    hypotheses, seed, group_offset)
    if not bool(ok[0]):
        return None, None, None
    return R[0], T[0], mask[0]


def _sift_chain(frames1, frames2, K, baseline_m, ratio_thresh, max_features, max_matches, hypotheses, seed, group_offset, roi1=None,
                roi2=None):
    """two clips -> (essential_ransac's result, x2d [2, T, max_matches, 2] NaN-padded, count [T]) on the device, no read-back"""
    dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _bgr_u8(frames1, dev), _bgr_u8(frames2, dev)
    if a.dim() != 4 or b.dim() != 4 or a.shape[0] != b.shape[0]:
        raise ValueError(f"estimate_camera_poses_from_SIFT: need two clips of T frames, got {list(a.shape)}, {list(b.shape)}")
    T_, mm = int(a.shape[0]), int(max_matches)
    box = lambda r: None if r is None else torch.as_tensor(np.asarray(r, dtype=np.float64)).reshape(T_, 4).to(dev)   # noqa: E731
    fa = geometry.sift_features(a, max_features, roi=box(roi1))
    fb = geometry.sift_features(b, max_features, roi=box(roi2))
    m = geometry.match_l2(fa.desc, fa.count, fb.desc, fb.count, ratio=ratio_thresh, max_matches=mm)
    r, x2d = _poses_from_matches(fa.xy, fb.xy, m.pairs, K, baseline_m, hypotheses, seed, group_offset)
    return r, x2d, m.count


def estimate_camera_poses_from_SIFT(frames1, frames2, K, baseline_m, ratio_thresh: float = 0.75, max_features: int = 3000,
                                    max_matches: int = 1000, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0):
    """Every frame pair of two clips in one pass on the device: frames1, frames2 (T, H, W, 3) RGB (float in [0, 1] or
    uint8; or (T, H, W) gray), K (3, 3) shared -> (R (T, 3, 3), T (T, 3, 1), pose_mask (T, max_matches) uint8, success (T,)
    bool) as host arrays.  SIFT-style features of both clips, the ratio-tested L2 matches by (distance, query), the first
    max_matches of them gathered into NaN-padded correspondences, one essential_ransac with a group per frame; pose_mask
    marks the matches (in that order) that are inliers in front of both cameras.  A frame without a pose has NaN in R and T.
    Frame f is bitwise what estimate_camera_pose_from_SIFT gives for it with the same seed and group_offset = f."""
    r, x2d, _ = _sift_chain(frames1, frames2, K, baseline_m, ratio_thresh, max_features, max_matches, hypotheses, seed, group_offset)
    T_, mm = int(x2d.shape[1]), int(x2d.shape[2])
    return (r.R.cpu().numpy(), r.t.cpu().numpy().reshape(T_, 3, 1), r.pose_mask.cpu().numpy().reshape(T_, mm),
            r.success.cpu().numpy())


def estimate_camera_pose_from_SIFT(img1, img2, K, baseline_m, ratio_thresh: float = 0.75, max_features: int = 3000,
                                   max_matches: int = 1000, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0):
    """img1, img2 (H, W, 3) RGB, float in [0, 1] or uint8 ((H, W) gray too), K (3, 3) -> (R (3, 3), T (3, 1), pts1 (n, 2), pts2
    (n, 2), mask_pose (n,) uint8) as host arrays with X2 = R X1 + T and ||T|| = baseline_m; pts are the n ratio-tested
    matches ordered by (distance, query), float64 (float32 in the reference), mask_pose marks those that are inliers in
    front of both cameras.  ValueError below 8 matches and when no essential matrix is found, as the reference raises."""
    r, x2d, count = _sift_chain(_one(img1), _one(img2), K, baseline_m, ratio_thresh, max_features, max_matches, hypotheses, seed,
                                group_offset)
    n = int(count[0])
    if n < 8:
        raise ValueError(f"estimate_camera_pose_from_SIFT: only {n} matches, too few for a pose")
    if not bool(r.success[0]):
        raise ValueError("estimate_camera_pose_from_SIFT: no essential matrix found")
    pts = x2d[:, 0, :n].cpu().numpy()
    return r.R[0].cpu().numpy(), r.t[0].cpu().numpy().reshape(3, 1), pts[0], pts[1], r.pose_mask.cpu().numpy().reshape(-1)[:n]


def estimate_pose_from_bbox_region(imgL, imgR, bboxL, bboxR, K, baseline_m, ratio_thresh: float = 0.75, max_features: int = 3000,
                                   max_matches: int = 1000, hypotheses: int = 1024, seed: int = 0, group_offset: int = 0):
    """The pose from the features inside a box of each image: bbox = [x1, y1, x2, y2], truncated to integers as the
    reference's crop is -> (R, T (3, 1), mask_pose (n,)); (I, 0, None) below 5 matches and three None when no essential
    matrix is found, as the reference returns.  The boxes go in as sift_features' roi, which keeps full-frame coordinates:
    the reference's crop-then-offset is folded in, and unlike a crop the features near the box edge see the pixels outside
    it."""
    trunc = lambda bb: [[float(int(v)) for v in np.asarray(bb, dtype=np.float64).reshape(4)]]   # noqa: E731
    r, _, count = _sift_chain(_one(imgL), _one(imgR), K, baseline_m, ratio_thresh, max_features, max_matches, hypotheses, seed,
                              group_offset, trunc(bboxL), trunc(bboxR))
    n = int(count[0])
    if n < 5:
        return np.eye(3), np.zeros((3, 1)), None
    if not bool(r.success[0]):
        return None, None, None
    return r.R[0].cpu().numpy(), r.t[0].cpu().numpy().reshape(3, 1), r.pose_mask.cpu().numpy().reshape(-1)[:n]
