"""Counterpart of triangulation/camera_position/camera_position.py's keypoint path with the reference's signature:

    estimate_camera_pose_from_kpt(pts1, pts2, K, baseline_m) -> (R, T (3, 1), mask_pose)        (camera_position.py:88-117)

cv2.findEssentialMat(RANSAC, prob 0.999, threshold 1.0) + cv2.recoverPose there; geometry.essential_ransac on the device
here (DESIGN §2 "Essential matrix": 1024 five-point hypotheses, all scored, no early termination).  The reference's callers
(triangulation/view_process/two_view.py, triangulation/estimate_camera_position.py) loop over the frames and call it once
per frame on the 17 keypoints; `estimate_camera_poses_from_kpts` takes all frames as per-frame groups of one call.  Left
out: the SIFT / ORB front ends of that module (they need cv2's detectors)."""
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
