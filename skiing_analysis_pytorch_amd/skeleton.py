"""The two 17-joint skeletons of the project and the conversion between them (reference: VideoPose3D/coco_hm36.py), plus
the skeleton tables of the ground-truth-free joint quality (fuse.compute_q_nogt, geometry.joint_quality), written as data.

coco_to_h36m / h36m_to_coco take a host array, computed here in NumPy, or a device tensor, handed to
geometry.convert_skeleton (csrc/skeleton.hip), which these host functions restate; rules: DESIGN §2 "Skeleton conversion".
Results are float64.
"""
from __future__ import annotations

import numpy as np

COCO = dict(NOSE=0, L_EYE=1, R_EYE=2, L_EAR=3, R_EAR=4, L_SHO=5, R_SHO=6, L_ELB=7, R_ELB=8, L_WRI=9, R_WRI=10, L_HIP=11,
            R_HIP=12, L_KNE=13, R_KNE=14, L_ANK=15, R_ANK=16)
H36M = dict(PEL=0, R_HIP=1, R_KNE=2, R_ANK=3, L_HIP=4, L_KNE=5, L_ANK=6, SPINE=7, THORAX=8, NECK=9, HEAD=10, L_SHO=11,
            L_ELB=12, L_WRI=13, R_SHO=14, R_ELB=15, R_WRI=16)
LIMBS = ("L_SHO", "R_SHO", "L_ELB", "R_ELB", "L_WRI", "R_WRI", "L_HIP", "R_HIP", "L_KNE", "R_KNE", "L_ANK", "R_ANK")
COCO_LIMB_IDX = [COCO[n] for n in LIMBS]          # the 12 joints both skeletons have
H36M_LIMB_IDX = [H36M[n] for n in LIMBS]

# ---- tables of the joint quality: edges as positions on the joint axis ----
# VideoPose3D/fuse/fuse_eval.py
H36M_EDGES = [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 6), (0, 7), (7, 8), (8, 9), (9, 10), (8, 11), (11, 12), (12, 13),
              (8, 14), (14, 15), (15, 16)]
# the 15 MHR-70 joints of the fused clips in the order of their ids (fuse/main_unity.py: TARGET_IDS)
MHR70_15_IDS = [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 41, 62, 69]
MHR70_15_NAMES = ["Bone_Eye_L", "Bone_Eye_R", "Upperarm_L", "Upperarm_R", "lowerarm_l", "lowerarm_r", "Thigh_L", "Thigh_R",
                  "calf_l", "calf_r", "Foot_L", "Foot_R", "Hand_R", "Hand_L", "neck_01"]
# metrics/true_data_compare.py BONE_EDGES (ids) as positions in MHR70_15_IDS
MHR70_15_BONE_IDS = [(69, 5), (5, 7), (7, 62), (69, 6), (6, 8), (8, 41), (69, 9), (9, 11), (11, 13), (69, 10), (10, 12), (12, 14),
                     (9, 10), (5, 6)]
MHR70_15_EDGES = [(MHR70_15_IDS.index(a), MHR70_15_IDS.index(b)) for a, b in MHR70_15_BONE_IDS]
COCO_EDGES = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12), (11, 12), (11, 13),
              (13, 15), (12, 14), (14, 16)]
# left / right joints by name, for fuse.body_side_bias (fuse/fuse.py:23-39)
LEFT_JOINTS = ("Upperarm_L", "lowerarm_l", "Hand_L", "Thigh_L", "calf_l", "Foot_L")
RIGHT_JOINTS = ("Upperarm_R", "lowerarm_r", "Hand_R", "Thigh_R", "calf_r", "Foot_R")
COCO_NAMES = ["nose", "eye_l", "eye_r", "ear_l", "ear_r", "shoulder_l", "shoulder_r", "elbow_l", "elbow_r", "wrist_l", "wrist_r",
              "hip_l", "hip_r", "knee_l", "knee_r", "ankle_l", "ankle_r"]
H36M_NAMES = ["pelvis", "hip_r", "knee_r", "ankle_r", "hip_l", "knee_l", "ankle_l", "spine", "thorax", "neck", "head",
              "shoulder_l", "elbow_l", "wrist_l", "shoulder_r", "elbow_r", "wrist_r"]


def _is_tensor(X) -> bool:
    return type(X).__module__.startswith("torch")


def _clip17(fn, X):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim not in (2, 3) or X.shape[-2] != 17 or X.shape[-1] not in (2, 3):
        raise ValueError(f"{fn}: need (17, C) or (T, 17, C) with C in (2, 3), got {list(X.shape)}")
    return (X[None] if X.ndim == 2 else X), X.ndim == 2


def coco_to_h36m(X_coco, synthesize_head: bool = True):
    """coco_hm36.py:74-142.  COCO-17 (17, C) or (T, 17, C), C = 2 or 3 -> H36M-17 of the same shape: pelvis, thorax and
    spine are midpoints, neck = nose, head = nose + 0.5 (nose - eye centre) if synthesize_head else nose."""
    if _is_tensor(X_coco):
        from . import geometry
        return geometry.convert_skeleton(X_coco, "coco_to_h36m", synthesize_head=synthesize_head)
    X, single = _clip17("coco_to_h36m", X_coco)
    out = np.full(X.shape, np.nan, dtype=np.float64)
    out[:, H36M_LIMB_IDX] = X[:, COCO_LIMB_IDX]
    nose = X[:, COCO["NOSE"]]
    pelvis = (X[:, COCO["L_HIP"]] + X[:, COCO["R_HIP"]]) * 0.5
    thorax = (X[:, COCO["L_SHO"]] + X[:, COCO["R_SHO"]]) * 0.5
    out[:, H36M["PEL"]], out[:, H36M["THORAX"]], out[:, H36M["SPINE"]] = pelvis, thorax, (pelvis + thorax) * 0.5
    out[:, H36M["NECK"]] = nose
    out[:, H36M["HEAD"]] = nose + 0.5 * (nose - (X[:, COCO["L_EYE"]] + X[:, COCO["R_EYE"]]) * 0.5) if synthesize_head else nose
    return out[0] if single else out


def h36m_to_coco(X_h36m, synthesize_face: bool = False, face_mode: str = "nan"):
    """coco_hm36.py:147-221.  H36M-17 -> COCO-17: nose = neck, eyes and ears NaN unless synthesize_face (or face_mode =
    "approx"), then placed from the head, the head-neck direction and the shoulder vector.  The reference's quirk is kept:
    the degenerate-shoulder test is on the CLIP MEAN of the shoulder width; under 1e-8 every frame uses (1, 0, 0)[:C]
    as its shoulder vector, offsets' scale included; a NaN mean takes the normal branch."""
    synthesize_face = bool(synthesize_face) or face_mode == "approx"
    if _is_tensor(X_h36m):
        from . import geometry
        return geometry.convert_skeleton(X_h36m, "h36m_to_coco", synthesize_face=synthesize_face)
    X, single = _clip17("h36m_to_coco", X_h36m)
    T, _, C = X.shape
    out = np.full(X.shape, np.nan, dtype=np.float64)
    out[:, COCO_LIMB_IDX] = X[:, H36M_LIMB_IDX]
    out[:, COCO["NOSE"]] = X[:, H36M["NECK"]]
    if synthesize_face and T:
        head, neck = X[:, H36M["HEAD"]], X[:, H36M["NECK"]]
        sv = X[:, H36M["L_SHO"]] - X[:, H36M["R_SHO"]]
        if np.sqrt((sv * sv).sum(axis=1)).mean() < 1e-8:
            sv = np.tile(np.array([1.0, 0.0, 0.0])[:C], (T, 1))
        w = np.sqrt((sv * sv).sum(axis=1, keepdims=True))
        side = sv / (w + 1e-9)
        up = head - neck
        up = up / (np.sqrt((up * up).sum(axis=1, keepdims=True)) + 1e-9)
        for name, ks, ku in (("L_EYE", 0.25, 0.15), ("R_EYE", -0.25, 0.15), ("L_EAR", 0.35, 0.10), ("R_EAR", -0.35, 0.10)):
            out[:, COCO[name]] = head + (ks * w) * side - (ku * w) * up
    return out[0] if single else out
