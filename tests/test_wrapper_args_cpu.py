"""No GPU: the public surface of geometry.py after its split into device/<kernel file>.py, the shared argument helpers of
_args.py on CPU tensors and NumPy arrays, and every wrapper's refusal of host tensors, which comes before the library is
touched.  The surface and refusal tests use geometry.<name> only: they describe the wrappers as they were before the split
as well."""
import importlib
from pathlib import Path

import numpy as np
import pytest
import torch

from skiing_analysis_pytorch_amd import _lib, geometry

PUBLIC_NAMES = [
    'BAResult', 'BA_MODES', 'BA_PLACEMENTS', 'BA_WEIGHT_KEYS', 'BevSkeletonResult', 'CALIB_PARAMS', 'CalibrationResult',
    'ClipQualityResult', 'EVAL_LDS_ELEMS', 'EVAL_MAX_EDGES', 'EVAL_MAX_JOINTS', 'EVAL_MAX_PAIRS', 'EmaResult',
    'EssentialResult', 'FUSE_DIAG_FIELDS', 'FUSE_MAX_JOINTS', 'FUSE_SCALE_MODES', 'FuseH36MResult', 'FuseViewsResult',
    'GroundTrackResult', 'H36M_EDGES', 'H36M_LEFT_BONES', 'H36M_LR_PAIRS', 'H36M_RIGHT_BONES', 'HOMOGRAPHY_STAT_FIELDS',
    'HomographyResult', 'ICPResult', 'JOINT_STAT_FIELDS', 'KIN_BASE_SERIES', 'KIN_LAYOUT_MHR70_15', 'KIN_LDS_FRAMES',
    'KIN_ROLES', 'KIN_SERIES', 'KIN_STAT_FIELDS', 'KinematicsResult', 'LENS_COEFF_COUNTS', 'LENS_MAX_CAMERAS',
    'LENS_MAX_ITERS', 'MHR70_15_EDGES', 'MHR70_15_LEFT_BONES', 'MHR70_15_LR_PAIRS', 'MHR70_15_RIGHT_BONES', 'PersonOrigin',
    'PoseErrorsResult', 'ProjectResult', 'RESECT_LOSSES', 'ROBUST_MAX_JOINTS', 'ROBUST_MAX_REFINE_ITERS',
    'ROBUST_MAX_VIEWS', 'RefineResult', 'ResectResult', 'RobustResult', 'SAVGOL_MAX_WIN', 'SCENE_MAX_PIXELS',
    'SavgolResult', 'SceneCloud', 'TRACK_FIELDS', 'TriageResult', 'UndistortResult', 'VIEW_STAT_FIELDS', 'ba_weights',
    'bev_skeleton', 'bundle_adjust', 'calib_free_mask', 'calibrate_camera', 'clip_quality', 'distort_points',
    'essential_ransac', 'estimate_normals', 'extrinsic_to_RT', 'five_point', 'fuse_h36m', 'fuse_views', 'ground_track',
    'homography_fit', 'homography_points', 'icp_correspondences', 'icp_point_to_plane', 'kin_max_turns', 'kinematics',
    'lens_coeffs', 'person_origin', 'person_stats', 'pose_encoding_to_extri_intri', 'pose_errors', 'project_points',
    'recenter_cameras', 'refine_cameras_points', 'relative_pose', 'resect_cameras', 'robust_launch', 'scale_intrinsics',
    'scene_launch', 'scene_point_cloud', 'smooth_ema', 'smooth_savgol', 'triage_launch', 'triangulate_joints',
    'triangulate_robust', 'triangulate_triage', 'undistort_keypoints_steps', 'undistort_points',
    'unproject_depth_map_to_point_map']


def test_geometry_keeps_its_public_names():
    assert len(PUBLIC_NAMES) == 103 and PUBLIC_NAMES == sorted(PUBLIC_NAMES)
    have = sorted(n for n in dir(geometry) if not n.startswith("_"))
    assert [n for n in PUBLIC_NAMES if n not in have] == []
    assert geometry._lib is _lib and callable(geometry._undistorted_f32)


# ---- the wrappers refuse host tensors before the library is touched ----------------------------------------------------
z = torch.zeros
K3 = np.eye(3)
HOST_CALLS = {
    "pose_encoding_to_extri_intri": lambda: geometry.pose_encoding_to_extri_intri(z(1, 2, 9), (14, 14)),
    "triangulate_joints": lambda: geometry.triangulate_joints(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3), z(1, 2, 17, 2)),
    "triangulate_triage": lambda: geometry.triangulate_triage(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3), z(1, 2, 17, 2)),
    "triangulate_robust": lambda: geometry.triangulate_robust(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3), z(1, 2, 17, 2)),
    "triage_launch": lambda: geometry.triage_launch(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3), z(1, 2, 17, 2), None, 0.3, 2.0),
    "robust_launch": lambda: geometry.robust_launch(z(1, 2, 3, 3), z(1, 2, 3, 3), z(1, 2, 3), z(1, 2, 17, 2), None, 0.3, 2.0, 2, 5,
                                                    False),
    "person_origin": lambda: geometry.person_origin(z(1, 4, 4, 3), z(1, 4), (4, 4)),
    "recenter_cameras": lambda: geometry.recenter_cameras(z(1, 2, 8), z(1, 2, 3, 4)),
    "scene_point_cloud": lambda: geometry.scene_point_cloud(z(1, 1, 4, 4, 3), z(1, 1, 4, 4), z(1, 1, 3, 4, 4), z(1, 1, 3, 4)),
    "estimate_normals": lambda: geometry.estimate_normals(z(64, 3)),
    "icp_correspondences": lambda: geometry.icp_correspondences(z(64, 3), z(64, 3)),
    "icp_point_to_plane": lambda: geometry.icp_point_to_plane(z(64, 3), z(64, 3)),
    "relative_pose": lambda: geometry.relative_pose(z(1, 2, 3, 3), z(1, 2, 3)),
    "resect_cameras": lambda: geometry.resect_cameras(z(8, 3), z(2, 8, 2)),
    "refine_cameras_points": lambda: geometry.refine_cameras_points(z(8, 3), z(2, 8, 2)),
    "essential_ransac": lambda: geometry.essential_ransac(z(2, 8, 2), z(2, 3, 3), hypotheses=16),
    "five_point": lambda: geometry.five_point(z(1, 5, 2), z(1, 5, 2)),
    "fuse_h36m": lambda: geometry.fuse_h36m(z(2, 17, 3), z(2, 17, 3)),
    "fuse_views": lambda: geometry.fuse_views(z(2, 17, 3), z(2, 17, 3), z(2, 17, 2), z(2, 17, 2), root_idx=0, left_hip_idx=4,
                                              right_hip_idx=1, left_shoulder_idx=11, right_shoulder_idx=14),
    "smooth_ema": lambda: geometry.smooth_ema(z(4, 17, 3)),
    "smooth_savgol": lambda: geometry.smooth_savgol(z(4, 17, 3)),
    "kinematics": lambda: geometry.kinematics(z(4, 15, 3)),
    "pose_errors": lambda: geometry.pose_errors(z(4, 17, 3), z(4, 17, 3)),
    "clip_quality": lambda: geometry.clip_quality(z(4, 17, 3)),
    "distort_points": lambda: geometry.distort_points(z(5, 2), K3, np.zeros(5)),
    "undistort_points": lambda: geometry.undistort_points(z(5, 2), K3, np.zeros(5)),
    "undistort_keypoints_steps": lambda: geometry.undistort_keypoints_steps(z(1, 2, 17, 2), z(1, 2, 3, 3), np.zeros(5)),
    "project_points": lambda: geometry.project_points(z(5, 3), K3, np.zeros(3), K3),
    "homography_fit": lambda: geometry.homography_fit(z(4, 2), z(4, 2)),
    "homography_points": lambda: geometry.homography_points(z(4, 2), z(3, 3)),
    "bev_skeleton": lambda: geometry.bev_skeleton(z(2, 17, 3), z(2, 2)),
    "ground_track": lambda: geometry.ground_track(z(4, 2)),
    "calibrate_camera": lambda: geometry.calibrate_camera(z(54, 2), z(3, 54, 2), (640, 480)),
}
# not in the table: unproject_depth_map_to_point_map and person_stats (the launch of person_origin) check nothing, and
# bundle_adjust takes host arrays and uploads them


@pytest.mark.parametrize("name", sorted(HOST_CALLS))
def test_wrapper_refuses_host_tensors(name, monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)             # a wrapper that reached the library would fail to find it,
    monkeypatch.setattr(_lib, "LIB_PATH", Path("no_such_dir") / "libskimi.so")      # with a message that names no wrapper
    with pytest.raises(_lib.SkimiError, match=name if not name.endswith("_launch") else "triangulate_"):
        HOST_CALLS[name]()


# ---- the helpers of _args.py ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def A():
    return importlib.import_module("skiing_analysis_pytorch_amd._args")


def test_device_check_names_the_function_and_the_argument(A):
    A.on_device("f", None, None)                       # absent optional arguments pass
    for bad in (torch.zeros(2), np.zeros(2), [1.0]):
        with pytest.raises(_lib.SkimiError, match="^f needs device tensors$"):
            A.on_device("f", None, bad)
    with pytest.raises(_lib.SkimiError, match=r"^f needs a device tensor$"):
        A.on_device("f", torch.zeros(2), what="a device tensor")
    with pytest.raises(_lib.SkimiError, match=r"^f needs device tensors \(conf is on cpu\)$"):
        A.on_device("f", points=None, conf=torch.zeros(2))
    with pytest.raises(_lib.SkimiError, match="g needs device tensors"):
        A.f64_dev("g", torch.zeros(2))
    with pytest.raises(_lib.SkimiError, match="g needs device tensors"):
        A.clips("g", np.zeros((4, 17, 3)))


def test_conversions_leave_a_conforming_tensor_alone(A):
    a = torch.arange(6.0, dtype=torch.float64).reshape(2, 3)
    assert A.to_dev(a) is a and A.contig_as(a, torch.float64) is a and A.upload_f64(a, a.device) is a
    assert A.to_dev(None) is None and A.contig_as(None) is None
    v = torch.arange(12.0, dtype=torch.float32).reshape(2, 6)[:, ::2]
    for got in (A.to_dev(v), A.contig_as(v, torch.float64), A.upload_f64(v.numpy(), a.device)):
        assert got.dtype == torch.float64 and got.is_contiguous() and torch.equal(got, v.double())
    assert A.contig_as(v).dtype == torch.float32 and A.contig_as(v).is_contiguous()
    h = A.host_f64(torch.tensor([[1, 2], [3, 4]], dtype=torch.int32).t())
    assert h.dtype == np.float64 and h.flags.c_contiguous and h.tolist() == [[1.0, 3.0], [2.0, 4.0]]
    assert A.host_ptr(None) is None and A.host_ptr(h) == h.ctypes.data


def test_shape_table_states_both_shapes(A):
    rows = (("K", torch.zeros(2, 3, 3), (2, 3, 3)), ("conf", None, (2, 8)), ("R0", torch.zeros(1, 2, 3), (1, 2, 3, 3)))
    A.shapes("f", rows[:2])
    with pytest.raises(ValueError, match=r"^f: R0 must be \[1, 2, 3, 3\], got \[1, 2, 3\]$"):
        A.shapes("f", rows)
    cpu = torch.device("cpu")
    with pytest.raises(_lib.SkimiError, match=r"f needs device tensors on one device \(K is on cpu\)"):
        A.shapes("f", rows, f32_on=cpu)                 # the strict form asks for the device first, row by row


def test_group_split(A):
    assert A.group_split(34, None) == (34, 1) and A.group_split(34, 17) == (17, 2)
    assert A.group_split(34, 16) == (16, 2)             # a size that does not divide N: the library refuses it, with its own message
    assert A.group_split(34, 0) == (0, 0) and A.group_split(34, -3) == (-3, 0) and A.group_split(0, None) == (0, 0)
    assert A.group_split(8, 16) == (16, 0)


def test_leading_axis_rule(A):
    a = torch.zeros(4, 17, 3)
    b, single = A.add_lead(a, 4)
    assert single and b.shape == (1, 4, 17, 3) and b.data_ptr() == a.data_ptr()
    c, single = A.add_lead(b, 4)
    assert not single and c is b
    d, single = A.add_lead(torch.zeros(3), 4)           # two axes short: left as it is for the caller's shape check
    assert not single and d.shape == (3,)
    r = A.strip_lead((b, b[..., 0]), True)
    assert r[0].shape == (4, 17, 3) and r[1].shape == (4, 17) and A.strip_lead((b,), False)[0] is b


def test_lengths_vector(A):
    cpu = torch.device("cpu")
    assert A.lengths("f", None, 3, cpu) is None
    for given in ([4, 0, 2], np.array([4, 0, 2]), torch.tensor([4, 0, 2])):
        got = A.lengths("f", given, 3, cpu)
        assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [4, 0, 2]
    for bad in ([4, 0], [[4, 0, 2]], []):
        with pytest.raises(ValueError, match=r"^f: lengths must be \[3\], got "):
            A.lengths("f", bad, 3, cpu)


def test_index_list(A):
    arr, n = A.index_list("f", "edges", ((0, 1), (1, 2)), 128)
    assert n == 2 and list(arr) == [0, 1, 1, 2]
    arr, n = A.index_list("f", "edges", (), 128)        # an empty list still gives the C side a pointer
    assert n == 0 and len(arr) == 1
    arr, n = A.index_list("f", "edges", [(2 ** 40, -2 ** 40)], 128)
    assert list(arr) == [2 ** 31 - 1, -2 ** 31]
    with pytest.raises(ValueError, match="^f: 3 lr_pairs, at most 2$"):
        A.index_list("f", "lr_pairs", [(0, 1)] * 3, 2)


def test_lens_coefficients_per_camera(A):
    one = geometry.lens_coeffs([0.1, 0.2, 0.0, 0.0, 0.3])
    for d in (one, geometry.lens_coeffs(np.array([[0.1, 0.2, 0.0, 0.0, 0.3]])), one[None]):      # [k], cv2's [1, k], [1, 12]
        got = A.per_camera_coeffs("f", d, 3)
        assert got.shape == (3, 12) and got.flags.c_contiguous and (got == one).all()
    two = geometry.lens_coeffs(np.arange(8.0).reshape(2, 4))
    assert (A.per_camera_coeffs("f", two, 2) == two).all()
    with pytest.raises(ValueError, match=r"^f: dist must be \[k\] or \[3, k\], got \[2, 12\]$"):
        A.per_camera_coeffs("f", two, 3)
    with pytest.raises(ValueError, match="dist must be"):
        A.per_camera_coeffs("f", np.zeros((1, 2, 12)), 2)


def test_camera_matrices(A):
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    assert A.camera_matrices("f", "K", K, None).shape == (1, 3, 3) and A.camera_matrices("f", "P", K, 4).shape == (4, 3, 3)
    with pytest.raises(ValueError, match="f: P holds 2 cameras, K holds 3"):
        A.camera_matrices("f", "P", np.stack([K, K]), 3)
    with pytest.raises(ValueError, match=r"f: K must be \[3, 3\] or \[C, 3, 3\], got \[3, 4\]"):
        A.camera_matrices("f", "K", np.zeros((3, 4)), None)
    with pytest.raises(ValueError, match="focal"):
        A.camera_matrices("f", "K", np.zeros((3, 3)), None)


def test_workspace_conventions(A):
    cpu = torch.device("cpu")
    assert A.workspace(cpu, 0, optional=True) is None and A.workspace(cpu, 24, optional=True).numel() == 24
    assert A.workspace(cpu, 0).numel() == 0 and A.workspace(cpu, 0, at_least=8).numel() == 8
    w = A.workspace(cpu, 40, at_least=8, as_f64=True)
    assert w.dtype == torch.float64 and w.numel() == 5 and A.workspace(cpu, 0, at_least=8, as_f64=True).numel() == 1
    assert A.workspace(cpu, 40).dtype == torch.uint8
    for alloc, dt in ((A.f64, torch.float64), (A.f32, torch.float32), (A.i32, torch.int32), (A.u8, torch.uint8)):
        t = alloc(cpu, 2, 0, 3)
        assert t.dtype == dt and t.shape == (2, 0, 3)


def test_frame_clips_need_uint8_device_frames(A):
    for bad in (torch.zeros(2, 4, 4, 3, dtype=torch.uint8), np.zeros((2, 4, 4, 3), np.uint8)):
        with pytest.raises(_lib.SkimiError, match="^f needs a uint8 "):
            A.frame_clip("f", bad)
