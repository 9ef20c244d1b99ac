"""ctypes binding of librgc_hip.so (the C-ABI declared in include/rgc_hip.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there is no CPU
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGC_HIP_LIB") or os.path.join(_HERE, "librgc_hip.so")  # RGC_HIP_LIB: developer override (A/B builds)

DIRECT27, DIRECT7, DIRECT1, DIRECT_RADIUS = 0, 1, 2, 3

K_GRID, K_KNN_COV, K_VOXEL, K_LINEARIZE, K_ERROR, K_FITNESS, K_KNN_COV_SRC, K_KNN_COOP, K_KNN_COOP_SRC, K_COUNT = range(10)

OK = 0
ERR_INVALID, ERR_HIP, ERR_TOO_FEW_POINTS, ERR_GRID_TOO_LARGE, ERR_NO_INPUT, ERR_NONFINITE, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7


class Params(C.Structure):
    _fields_ = [("voxel_res", C.c_double), ("max_iterations", C.c_int), ("lm_max_iterations", C.c_int),
                ("rotation_eps", C.c_double), ("translation_eps", C.c_double), ("lm_init_lambda_factor", C.c_double),
                ("k_correspondences", C.c_int), ("neighbor_method", C.c_int), ("max_cells", C.c_longlong)]


class Stats(C.Structure):
    _fields_ = [("n_source", C.c_int), ("n_target", C.c_int), ("n_voxels", C.c_int), ("n_corr", C.c_int),
                ("outer_iterations", C.c_int), ("n_linearize", C.c_int), ("n_error", C.c_int),
                ("target_cells", C.c_longlong), ("source_cells", C.c_longlong),
                ("deferred_target", C.c_int), ("deferred_source", C.c_int), ("source_crowding", C.c_double),
                ("lazy_misses", C.c_int), ("searched_target", C.c_int), ("lm_fallbacks", C.c_int)]


class FuseIn(C.Structure):
    _fields_ = [("q_lidar_xyzw", C.c_double * 4), ("t_lidar", C.c_double * 3), ("fitness", C.c_double), ("use_ground", C.c_int),
                ("ground_last", C.c_double * 11), ("ground_cur", C.c_double * 11), ("q_w_curr_f_xyzw", C.c_double * 4),
                ("ground_cov", C.c_double), ("use_imu", C.c_int), ("q_imu_xyzw", C.c_double * 4), ("max_iterations", C.c_int)]


class ImuFilter(C.Structure):
    _fields_ = [("ba", C.c_double * 3), ("bg", C.c_double * 3), ("dropped", C.c_int), ("count", C.c_int), ("t_last", C.c_double),
                ("roll", C.c_double), ("pitch", C.c_double), ("yaw", C.c_double), ("roll_last", C.c_double), ("pitch_last", C.c_double),
                ("Rwi", C.c_double * 9), ("mf_buf", (C.c_double * 201) * 3), ("mf_count", C.c_int * 3)]


class GroundGate(C.Structure):
    _fields_ = [("gflag", C.c_int), ("changegroundflag", C.c_int), ("q_w_curr_delta", C.c_double * 4), ("n_history", C.c_int),
                ("history", (C.c_double * 4) * 64)]


class FeParams(C.Structure):
    _fields_ = [("n_scans", C.c_int), ("min_range", C.c_double), ("max_range", C.c_double), ("use_intensity", C.c_int)]


class FeOut(C.Structure):
    _fields_ = [("cloud", C.POINTER(C.c_float)), ("cloud_cap", C.c_int), ("n_cloud", C.c_int), ("sharp", C.POINTER(C.c_float)),
                ("flat", C.POINTER(C.c_float)), ("inten", C.POINTER(C.c_float)), ("feat_cap", C.c_int), ("n_sharp", C.c_int),
                ("n_sharp_own", C.c_int), ("n_flat", C.c_int), ("n_inten", C.c_int), ("ground_pts", C.POINTER(C.c_float)),
                ("ground_cap", C.c_int), ("n_ground", C.c_int), ("groundparam", C.c_double * 11), ("ground_valid", C.c_int),
                ("ring_count", C.c_int * 64), ("curvature", C.POINTER(C.c_float)), ("curvature2", C.POINTER(C.c_float)),
                ("inten_curvature", C.POINTER(C.c_float)), ("label", C.POINTER(C.c_int)), ("inten_label", C.POINTER(C.c_int)),
                ("picked", C.POINTER(C.c_int)), ("ground_marked", C.POINTER(C.c_int))]


class MapregReport(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int), ("successful", C.c_int),
                ("n_edge_cur", C.c_int), ("n_plane_cur", C.c_int), ("n_edge_last", C.c_int), ("n_plane_last", C.c_int)]


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double),
                ("euclidean_fitness_epsilon", C.c_double)]


class IcpResult(C.Structure):
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("state", C.c_int), ("n_correspondences", C.c_int), ("fitness", C.c_double)]


class Pc2Layout(C.Structure):
    _fields_ = [("point_step", C.c_int), ("offset", C.c_int * 6), ("datatype", C.c_int * 6), ("is_bigendian", C.c_int), ("strict", C.c_int)]


class Pc2Field(C.Structure):
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_int), ("datatype", C.c_int), ("count", C.c_int)]


class MapregGround(C.Structure):
    _fields_ = [("last_v1", C.c_double * 3), ("last_v2", C.c_double * 3), ("last_norm", C.c_double * 3), ("last_distance", C.c_double),
                ("cur_norm", C.c_double * 3), ("cur_distance", C.c_double), ("q_history", C.c_double * 4), ("last_q", C.c_double * 4),
                ("last_t", C.c_double * 3), ("p_var", C.c_double)]


class MapregImu(C.Structure):
    _fields_ = [("delta_q", C.c_double * 4), ("imu_cov", C.c_double), ("pitch_cur", C.c_double), ("roll_cur", C.c_double),
                ("pitch_last", C.c_double), ("roll_last", C.c_double), ("pr_var", C.c_double)]


class MapInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_int), ("n_points", C.c_longlong), ("n_target", C.c_int), ("revision", C.c_ulonglong),
                ("oldest_id", C.c_int), ("newest_id", C.c_int), ("origin", C.c_double * 3)]


class KfPose(C.Structure):
    """rgc_kf_pose: PointXYZIRPYT's pose fields, radians"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("roll", C.c_float), ("pitch", C.c_float), ("yaw", C.c_float)]


class KfInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_int), ("n_points", C.c_longlong * 3), ("revision", C.c_ulonglong)]


KF_CORNER, KF_SURF, KF_SCAN, KF_KINDS = 0, 1, 2, 3


class KfLoopParams(C.Structure):
    """rgc_kf_loop_params: the constants of detectLoopClosure (rgc_default_kf_loop_params)"""
    _fields_ = [("history_search_radius", C.c_float), ("drift_factor", C.c_float), ("distance_by_loop", C.c_float), ("loop_keyframe_dis_diff", C.c_float),
                ("history_search_num", C.c_int), ("min_key_id", C.c_int)]


class KfLoopCandidate(C.Structure):
    """rgc_kf_loop_candidate: what rgc_kf_detect_loop found"""
    _fields_ = [("found", C.c_int), ("latest_id", C.c_int), ("closest_id", C.c_int), ("latest_pose", KfPose), ("closest_pose", KfPose),
                ("search_radius", C.c_float), ("n_in_radius", C.c_int)]


class PgoLoop(C.Structure):
    """rgc_pgo_loop: one loop edge of the 4-DoF pose graph (key_loop -> key_curr)"""
    _fields_ = [("key_curr", C.c_int), ("key_loop", C.c_int), ("t_loop_curr", C.c_double * 3), ("yaw_loop_curr_deg", C.c_double),
                ("pitch_loop_deg", C.c_double), ("roll_loop_deg", C.c_double)]


class PgoParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("initial_radius", C.c_double)]


class PgoReport(C.Structure):
    _fields_ = [("status", C.c_int), ("n_nodes", C.c_int), ("n_odom", C.c_int), ("n_loops_used", C.c_int), ("n_loops_ignored", C.c_int),
                ("fixed_id", C.c_int), ("iterations", C.c_int), ("successful", C.c_int), ("stop", C.c_int), ("accepted_mask", C.c_uint),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


PGO_OPTIMIZED, PGO_NO_LOOP = 0, 1
PGO_STOP_CAP, PGO_STOP_GRADIENT, PGO_STOP_FUNCTION, PGO_STOP_PARAMETER, PGO_STOP_RADIUS = range(5)
PGO_MAX_LOOPS = 128


class VgRoute(C.Structure):
    """rgc_vg_route: what the last leaf filter on a context did (rgc_voxelgrid_route)"""
    _fields_ = [("path", C.c_int), ("status", C.c_int), ("repeated", C.c_int), ("kept_box", C.c_int), ("kept_flags", C.c_int), ("box_invalidated", C.c_int),
                ("chain", C.c_int), ("leaf_buckets", C.c_int), ("seg_shift", C.c_int), ("nseg", C.c_int), ("packed", C.c_int), ("edge", C.c_int), ("flags", C.c_int),
                ("minb", C.c_int * 3), ("div", C.c_int * 3), ("n", C.c_int), ("n_out", C.c_int)]


class NdtParams(C.Structure):
    """rgc_ndt_params: the settings of the NDT registration (rgc_ndt_set_params)"""
    _fields_ = [("resolution", C.c_double), ("distance_mode", C.c_int), ("neighbor_method", C.c_int), ("neighbor_radius", C.c_double)]


class GicpMpParams(C.Structure):
    """rgc_gicp_mp_params: the settings of FastGICPMultiPoints (rgc_gicpmp_set_params)"""
    _fields_ = [("neighbor_search_radius", C.c_double), ("max_iterations", C.c_int), ("rotation_epsilon", C.c_double), ("transformation_epsilon", C.c_double)]


class SearchInfo(C.Structure):
    """rgc_search_info: the search index and what its last query call cost (rgc_search_get_info)"""
    _fields_ = [("n", C.c_int), ("cell", C.c_double), ("cells", C.c_longlong), ("candidates", C.c_longlong), ("grown", C.c_int), ("rows_sorted_long", C.c_int)]


SEARCH_MAX_K = 32


class OutlierInfo(C.Structure):
    """rgc_outlier_info: the last outlier filter call (rgc_outlier_get_info)"""
    _fields_ = [("n", C.c_int), ("n_out", C.c_int), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("cell", C.c_double),
                ("cells", C.c_longlong), ("candidates", C.c_longlong), ("grown", C.c_int)]


OUTLIER_MAX_MEAN_K = 63


class ClusterInfo(C.Structure):
    """rgc_cluster_info: the last rgc_cluster_extract (rgc_cluster_get_info)"""
    _fields_ = [("n", C.c_int), ("n_components", C.c_int), ("n_clusters", C.c_int), ("n_clustered", C.c_int), ("largest", C.c_int), ("cell", C.c_double),
                ("cells", C.c_longlong), ("candidates", C.c_longlong)]


class PlaneParams(C.Structure):
    """rgc_plane_params (rgc_default_plane_params)"""
    _fields_ = [("distance_threshold", C.c_double), ("probability", C.c_double), ("eps_angle", C.c_double), ("axis", C.c_double * 3), ("seed", C.c_ulonglong),
                ("max_iterations", C.c_int), ("optimize", C.c_int), ("model_type", C.c_int), ("reserved", C.c_int)]


class PlaneInfo(C.Structure):
    """rgc_plane_info: the last rgc_plane_segment (rgc_plane_get_info)"""
    _fields_ = [("n", C.c_int), ("n_inliers", C.c_int), ("iterations", C.c_int), ("best_count", C.c_int), ("batch", C.c_int), ("launches", C.c_int), ("refined", C.c_int),
                ("reserved", C.c_int), ("positions", C.c_longlong), ("skipped", C.c_longlong), ("best_position", C.c_longlong), ("k", C.c_double),
                ("ransac_coeff", C.c_double * 4)]


PLANE_PLANE, PLANE_PERPENDICULAR = 0, 1
PLANE_MAX_BATCH = 1024


class NormalParams(C.Structure):
    """rgc_normal_params (rgc_default_normal_params)"""
    _fields_ = [("k", C.c_int), ("flip", C.c_int), ("radius", C.c_double), ("viewpoint", C.c_float * 3), ("reserved", C.c_int)]


class NormalInfo(C.Structure):
    """rgc_normal_info: the last rgc_normal_estimate (rgc_normal_get_info)"""
    _fields_ = [("n", C.c_int), ("n_surface", C.c_int), ("n_valid", C.c_int), ("route", C.c_int), ("cell", C.c_double), ("cells", C.c_longlong),
                ("candidates", C.c_longlong), ("grown", C.c_int), ("reserved", C.c_int)]


NORMAL_MAX_K = 32
NORMAL_ROUTE_K, NORMAL_ROUTE_RADIUS = 0, 1


class FpfhParams(C.Structure):
    """rgc_fpfh_params (rgc_default_fpfh_params)"""
    _fields_ = [("radius", C.c_double), ("reserved", C.c_int * 2)]


class FpfhInfo(C.Structure):
    """rgc_fpfh_info: the last rgc_fpfh_estimate (rgc_fpfh_get_info)"""
    _fields_ = [("n", C.c_int), ("n_surface", C.c_int), ("n_valid", C.c_int), ("n_spfh", C.c_int), ("cell", C.c_double), ("cells", C.c_longlong),
                ("pairs", C.c_longlong), ("candidates", C.c_longlong), ("reserved", C.c_int * 2)]


FPFH_BINS = 33

NDT_P2D, NDT_D2D = 0, 1
NDT_DIRECT27, NDT_DIRECT7, NDT_DIRECT1, NDT_DIRECT_RADIUS = 0, 1, 2, 3
NDT_MAX_OFFSETS = 512

VG_PATH_NONE, VG_PATH_KEPT, VG_PATH_MEASURED, VG_PATH_UNFILTERED = 0, 1, 2, 3


class RgcError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"rgc_hip status {status}: {msg}")
        self.status = status


# every symbol include/rgc_hip.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "rgc_default_params", "rgc_create", "rgc_destroy", "rgc_set_params", "rgc_get_params", "rgc_neighbor_offsets", "rgc_set_neighbor_search", "rgc_get_neighbor_search", "rgc_last_error",
    "rgc_status_string", "rgc_version", "rgc_set_target", "rgc_set_source", "rgc_set_target_device",
    "rgc_set_source_device", "rgc_linearize", "rgc_compute_error", "rgc_num_correspondences", "rgc_align", "rgc_align_begin", "rgc_align_end", "rgc_align_end_reframe", "rgc_share_target", "rgc_hold_source_until_target_of", "rgc_set_target_lazy", "rgc_set_knn_reuse", "rgc_get_knn_reuse", "rgc_set_regularization_method", "rgc_set_voxel_accumulation_mode",
    "rgc_set_covariance_estimation", "rgc_get_covariance_estimation", "rgc_set_rbf_kernel", "rgc_get_rbf_kernel",
    "rgc_fitness", "rgc_get_aligned", "rgc_get_aligned_device", "rgc_get_source_covariances", "rgc_get_target_covariances", "rgc_set_source_covariances", "rgc_set_target_covariances",
    "rgc_clear_source", "rgc_clear_target", "rgc_swap_source_and_target", "rgc_get_voxels",
    "rgc_get_stats", "rgc_device_alloc", "rgc_device_free", "rgc_host_alloc", "rgc_host_free", "rgc_upload", "rgc_download", "rgc_synchronize",
    "rgc_stream", "rgc_default_fe_params", "rgc_frontend", "rgc_extract_pose", "rgc_imu_preintegrate", "rgc_imu_filter_init", "rgc_imu_filter_push", "rgc_ground_gate_init", "rgc_ground_gate_remember", "rgc_ground_gate_step", "rgc_default_fuse_in", "rgc_fuse_pose", "rgc_compose_pose",
    "rgc_R2ypr", "rgc_ypr2R", "rgc_deskew", "rgc_voxelgrid", "rgc_voxelgrid_begin", "rgc_voxelgrid_end", "rgc_voxelgrid_route", "rgc_uniform_sampling", "rgc_transform_cloud", "rgc_set_target_reframed", "rgc_frontend_device", "rgc_frontend_cloud_device", "rgc_default_icp_params", "rgc_icp_align", "rgc_pc2_unpack", "rgc_pc2_pack", "rgc_pc2_point_fields", "rgc_tum_line", "rgc_pcd_write", "rgc_mapreg_set_maps", "rgc_mapreg_associate", "rgc_mapreg_optimize", "rgc_mapreg_linearize", "rgc_map_reset", "rgc_map_insert", "rgc_map_evict", "rgc_map_rebase", "rgc_map_commit", "rgc_map_get_info", "rgc_map_download", "rgc_kf_reset", "rgc_kf_push", "rgc_kf_set_poses", "rgc_kf_get_info", "rgc_kf_assemble", "rgc_kf_get_travel", "rgc_kf_select_surrounding", "rgc_kf_select_global", "rgc_default_kf_loop_params", "rgc_kf_detect_loop", "rgc_mapreg_set_maps_device", "rgc_icp_align_device",
    "rgc_default_pgo_params", "rgc_pgo_make_loop", "rgc_pgo_optimize", "rgc_pgo_linearize",
    "rgc_default_ndt_params", "rgc_ndt_set_params", "rgc_ndt_get_params", "rgc_ndt_set_target", "rgc_ndt_set_source", "rgc_ndt_set_target_device", "rgc_ndt_set_source_device", "rgc_ndt_clear_source", "rgc_ndt_clear_target", "rgc_ndt_swap_source_and_target", "rgc_ndt_linearize", "rgc_ndt_compute_error", "rgc_ndt_num_correspondences", "rgc_ndt_align", "rgc_ndt_get_voxels", "rgc_ndt_get_raw_covariances",
    "rgc_gicp_set_max_correspondence_distance", "rgc_gicp_get_max_correspondence_distance", "rgc_gicp_linearize", "rgc_gicp_compute_error", "rgc_gicp_num_correspondences", "rgc_gicp_get_correspondences", "rgc_gicp_align",
    "rgc_gicpst_reset", "rgc_gicpst_linearize", "rgc_gicpst_compute_error", "rgc_gicpst_num_correspondences", "rgc_gicpst_num_searched", "rgc_gicpst_get_correspondences", "rgc_gicpst_align",
    "rgc_default_gicp_mp_params", "rgc_gicpmp_set_params", "rgc_gicpmp_get_params", "rgc_gicpmp_linearize", "rgc_gicpmp_num_correspondences", "rgc_gicpmp_num_candidates", "rgc_gicpmp_get_merged", "rgc_gicpmp_get_neighbors", "rgc_gicpmp_align",
    "rgc_search_set_cloud", "rgc_search_clear", "rgc_search_get_info", "rgc_search_sort_window", "rgc_search_knn", "rgc_search_radius",
    "rgc_outlier_statistical", "rgc_outlier_radius", "rgc_outlier_get_info", "rgc_outlier_set_cell",
    "rgc_cluster_extract", "rgc_cluster_get_info", "rgc_cluster_set_cell",
    "rgc_default_plane_params", "rgc_plane_segment", "rgc_plane_get_info", "rgc_plane_set_batch", "rgc_plane_sample",
    "rgc_default_normal_params", "rgc_normal_estimate", "rgc_normal_get_info", "rgc_normal_set_cell",
    "rgc_default_fpfh_params", "rgc_fpfh_estimate", "rgc_fpfh_get_info", "rgc_fpfh_set_cell",
    "rgc_profile_enable", "rgc_profile_select", "rgc_profile_reset", "rgc_profile_get", "rgc_profile_name",
]

_lib = None


class _PartialLibrary:
    """RGC_HIP_LIB_PARTIAL=1: LIB_PATH names a library built from a SUBSET of the sources -- csrc/rgc_host.cpp alone under
    -fsanitize=address,undefined (tests/test_sanitizers.py: the scalar host stages need no HIP).  A symbol it lacks becomes a stand-in
    that takes the prototype declarations below and raises when called; the product library is never loaded this way."""

    class _Missing:
        def __init__(self, name):
            object.__setattr__(self, "_name", name)

        def __setattr__(self, k, v):
            pass

        def __call__(self, *a, **kw):
            raise RuntimeError(f"{self._name} is not in the partial library {LIB_PATH}")

    def __init__(self, real):
        self._real = real
        self._missing = {}

    def __getattr__(self, name):
        try:
            return getattr(self._real, name)
        except AttributeError:
            return self._missing.setdefault(name, _PartialLibrary._Missing(name))


_seq = None


def load_seq():
    """librgc_seq.so: the C++ host layer's dependent frame loop behind one call (cpp/dependent_sequence_c.cpp).  It is linked against the
    in-tree librgc_hip.so; with RGC_HIP_LIB naming another build there is no frame loop for it (None): contexts of one library build
    must not be driven through another's code."""
    global _seq
    if _seq is not None:
        return _seq
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "librgc_seq.so")
    if os.path.abspath(LIB_PATH) != os.path.join(os.path.dirname(os.path.abspath(__file__)), "librgc_hip.so") or not os.path.exists(path):
        return None
    load()
    S = C.CDLL(path)
    vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    S.rgc_seq_run_dependent.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.POINTER(vp), ip, C.c_int, C.c_int, dp, fp, C.c_int, fp, dp, dp, ip, dp]
    S.rgc_seq_run_dependent.restype = C.c_int
    _seq = S
    return S


def load():
    """Load librgc_hip.so and declare prototypes.  Raises if the library is missing (build with
    `python rgc-slam_amd/build.py` or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback); "
                          f"run `python rgc-slam_amd/build.py`")
    L = C.CDLL(LIB_PATH)
    if os.environ.get("RGC_HIP_LIB_PARTIAL") == "1":
        L = _PartialLibrary(L)
    vp, fp, dp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.rgc_default_params.argtypes = [C.POINTER(Params)]
    L.rgc_default_params.restype = None
    L.rgc_create.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(vp)]
    L.rgc_destroy.argtypes = [vp]
    L.rgc_destroy.restype = None
    L.rgc_set_params.argtypes = [vp, C.POINTER(Params)]
    L.rgc_get_params.argtypes = [vp, C.POINTER(Params)]
    L.rgc_neighbor_offsets.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.rgc_set_neighbor_search.argtypes = [vp, C.c_int, C.c_double]
    L.rgc_get_neighbor_search.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.rgc_last_error.argtypes = [vp]
    L.rgc_last_error.restype = C.c_char_p
    L.rgc_status_string.argtypes = [C.c_int]
    L.rgc_status_string.restype = C.c_char_p
    L.rgc_version.restype = C.c_char_p
    for f in (L.rgc_set_target, L.rgc_set_source, L.rgc_set_target_device, L.rgc_set_source_device):
        f.argtypes = [vp, vp, C.c_int, C.c_int]
    L.rgc_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.rgc_compute_error.argtypes = [vp, dp, dp]
    L.rgc_num_correspondences.argtypes = [vp, ip]
    L.rgc_align.argtypes = [vp, fp, fp, dp, dp, ip, ip, ip]
    L.rgc_align_begin.argtypes = [vp, fp, C.c_int]
    L.rgc_align_end.argtypes = [vp, fp, dp, dp, ip, ip, ip]
    L.rgc_share_target.argtypes = [vp, vp]
    L.rgc_fitness.argtypes = [vp, fp, dp]
    L.rgc_get_aligned.argtypes = [vp, fp, fp, C.c_int]
    L.rgc_get_aligned_device.argtypes = [vp, fp, vp, C.c_int]
    L.rgc_get_source_covariances.argtypes = [vp, dp, dp]
    L.rgc_set_source_covariances.argtypes = [vp, dp, C.c_int]
    L.rgc_set_target_covariances.argtypes = [vp, dp, C.c_int]
    L.rgc_hold_source_until_target_of.argtypes = [vp, vp]
    L.rgc_set_target_lazy.argtypes = [vp, C.c_int]
    L.rgc_set_knn_reuse.argtypes = [vp, C.c_int]
    L.rgc_set_regularization_method.argtypes = [vp, C.c_int]
    L.rgc_set_voxel_accumulation_mode.argtypes = [vp, C.c_int]
    L.rgc_set_covariance_estimation.argtypes = [vp, C.c_int]
    L.rgc_get_covariance_estimation.argtypes = [vp, C.POINTER(C.c_int)]
    L.rgc_set_rbf_kernel.argtypes = [vp, C.c_double, C.c_double]
    L.rgc_get_rbf_kernel.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rgc_get_knn_reuse.argtypes = [vp, ip]
    L.rgc_clear_source.argtypes = [vp]
    L.rgc_clear_target.argtypes = [vp]
    L.rgc_swap_source_and_target.argtypes = [vp]
    L.rgc_get_target_covariances.argtypes = [vp, dp, dp]
    L.rgc_get_voxels.argtypes = [vp, C.c_int, ip, ip, dp, dp, ip]
    L.rgc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.rgc_align_end_reframe.argtypes = [vp, vp, dp, vp, C.c_int, C.c_int, vp, C.POINTER(C.c_float), dp, dp, ip, ip, ip]
    L.rgc_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.rgc_device_free.argtypes = [vp, vp]
    L.rgc_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.rgc_host_free.argtypes = [vp]
    L.rgc_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.rgc_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.rgc_synchronize.argtypes = [vp]
    L.rgc_stream.argtypes = [vp]
    L.rgc_stream.restype = vp
    L.rgc_default_fe_params.argtypes = [C.POINTER(FeParams)]
    L.rgc_default_fe_params.restype = None
    L.rgc_frontend.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(FeParams), C.POINTER(FeOut)]
    L.rgc_frontend_device.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(FeParams), C.POINTER(FeOut)]
    L.rgc_extract_pose.argtypes = [fp, dp, dp]
    L.rgc_imu_preintegrate.argtypes = [dp, dp, dp, C.c_int, C.c_double, C.c_double, dp, dp, dp, dp]
    L.rgc_imu_filter_init.argtypes = [C.POINTER(ImuFilter)]
    L.rgc_imu_filter_init.restype = None
    L.rgc_imu_filter_push.argtypes = [C.POINTER(ImuFilter), C.c_double, dp, dp, dp, dp]
    L.rgc_ground_gate_init.argtypes = [C.POINTER(GroundGate)]
    L.rgc_ground_gate_init.restype = None
    L.rgc_ground_gate_remember.argtypes = [C.POINTER(GroundGate)]
    L.rgc_ground_gate_remember.restype = None
    L.rgc_ground_gate_step.argtypes = [C.POINTER(GroundGate), dp, dp, dp, dp, dp, dp, dp]
    L.rgc_default_fuse_in.argtypes = [C.POINTER(FuseIn)]
    L.rgc_default_fuse_in.restype = None
    L.rgc_fuse_pose.argtypes = [C.POINTER(FuseIn), dp, dp, ip]
    L.rgc_compose_pose.argtypes = [dp, dp, dp, dp, dp, C.c_int, dp, dp, dp, dp]
    L.rgc_R2ypr.argtypes = [dp, dp]
    L.rgc_R2ypr.restype = None
    L.rgc_ypr2R.argtypes = [dp, dp]
    L.rgc_ypr2R.restype = None
    L.rgc_deskew.argtypes = [vp, vp, C.c_int, C.c_int, dp, dp, C.c_int]
    L.rgc_voxelgrid.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, vp, ip, C.c_int]
    L.rgc_voxelgrid_begin.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, vp]
    L.rgc_voxelgrid_end.argtypes = [vp, ip]
    L.rgc_voxelgrid_route.argtypes = [vp, C.POINTER(VgRoute)]
    L.rgc_uniform_sampling.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, ip, C.c_int]
    L.rgc_transform_cloud.argtypes = [vp, vp, C.c_int, C.c_int, dp, dp, vp, C.c_int]
    L.rgc_set_target_reframed.argtypes = [vp, vp, C.c_int, C.c_int, dp, dp, vp]
    L.rgc_default_icp_params.argtypes = [C.POINTER(IcpParams)]
    L.rgc_default_icp_params.restype = None
    L.rgc_icp_align.argtypes = [vp, fp, C.c_int, fp, C.c_int, C.c_int, C.POINTER(IcpParams), fp, C.POINTER(IcpResult)]
    L.rgc_pc2_unpack.argtypes = [vp, vp, C.c_int, C.POINTER(Pc2Layout), vp, vp, vp, C.c_int]
    L.rgc_pc2_pack.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp]
    L.rgc_pc2_point_fields.argtypes = [C.c_int, C.POINTER(Pc2Field), C.c_int, ip]
    L.rgc_tum_line.argtypes = [C.c_double, dp, dp, C.c_char_p, C.c_int]
    L.rgc_pcd_write.argtypes = [C.c_char_p, fp, C.c_int, C.c_int]
    L.rgc_mapreg_set_maps.argtypes = [vp, fp, C.c_int, fp, C.c_int, C.c_int]
    L.rgc_mapreg_associate.argtypes = [vp, C.c_int, fp, C.c_int, dp, dp, dp, ip]
    L.rgc_mapreg_optimize.argtypes = [vp, fp, C.c_int, fp, C.c_int, fp, C.c_int, fp, C.c_int, C.POINTER(MapregGround), C.POINTER(MapregGround),
                                      C.POINTER(MapregImu), dp, C.POINTER(MapregReport), ip]
    L.rgc_mapreg_linearize.argtypes = [vp, fp, C.c_int, fp, C.c_int, fp, C.c_int, fp, C.c_int, C.POINTER(MapregGround), C.POINTER(MapregGround),
                                       C.POINTER(MapregImu), dp, dp, dp, dp, dp, ip, C.POINTER(dp)]
    L.rgc_frontend_cloud_device.argtypes = [vp, C.POINTER(C.c_void_p), ip]
    L.rgc_map_reset.argtypes = [vp, dp]
    L.rgc_map_insert.argtypes = [vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, ip]
    L.rgc_map_evict.argtypes = [vp, C.c_int, dp, C.c_double, ip]
    L.rgc_map_rebase.argtypes = [vp, dp]
    L.rgc_map_commit.argtypes = [vp, C.c_float, ip]
    L.rgc_map_get_info.argtypes = [vp, C.POINTER(MapInfo)]
    L.rgc_map_download.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    L.rgc_kf_reset.argtypes = [vp]
    L.rgc_kf_push.argtypes = [vp, C.c_int, C.POINTER(KfPose), vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int]
    L.rgc_kf_set_poses.argtypes = [vp, ip, C.POINTER(KfPose), C.c_int]
    L.rgc_kf_get_info.argtypes = [vp, C.POINTER(KfInfo)]
    L.rgc_kf_assemble.argtypes = [vp, ip, C.c_int, C.c_uint, C.c_float, vp, C.c_int, C.c_int, ip, ip]
    L.rgc_kf_get_travel.argtypes = [vp, ip, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rgc_kf_select_surrounding.argtypes = [vp, C.POINTER(C.c_float), C.c_float, C.c_float, ip, C.c_int, ip, ip]
    L.rgc_kf_select_global.argtypes = [vp, C.c_float, ip, C.c_int, ip]
    L.rgc_default_kf_loop_params.argtypes = [C.POINTER(KfLoopParams)]
    L.rgc_default_kf_loop_params.restype = None
    L.rgc_kf_detect_loop.argtypes = [vp, C.POINTER(KfLoopParams), C.POINTER(KfLoopCandidate), ip, C.c_int, ip]
    L.rgc_mapreg_set_maps_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int]
    L.rgc_icp_align_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(IcpParams), fp, C.POINTER(IcpResult)]
    L.rgc_default_pgo_params.argtypes = [C.POINTER(PgoParams)]
    L.rgc_default_pgo_params.restype = None
    L.rgc_pgo_make_loop.argtypes = [C.POINTER(KfPose), C.POINTER(KfPose), fp, C.c_int, C.c_int, C.POINTER(PgoLoop)]
    L.rgc_pgo_optimize.argtypes = [vp, ip, C.c_int, C.POINTER(PgoLoop), C.c_int, C.POINTER(PgoParams), C.c_int, C.POINTER(KfPose), C.POINTER(PgoReport)]
    L.rgc_pgo_linearize.argtypes = [vp, ip, C.c_int, C.POINTER(PgoLoop), C.c_int, dp, C.c_double, ip, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(PgoReport)]
    L.rgc_default_ndt_params.argtypes = [C.POINTER(NdtParams)]
    L.rgc_default_ndt_params.restype = None
    L.rgc_ndt_set_params.argtypes = [vp, C.POINTER(NdtParams)]
    L.rgc_ndt_get_params.argtypes = [vp, C.POINTER(NdtParams)]
    for f in (L.rgc_ndt_set_target, L.rgc_ndt_set_source, L.rgc_ndt_set_target_device, L.rgc_ndt_set_source_device):
        f.argtypes = [vp, vp, C.c_int, C.c_int]
    for f in (L.rgc_ndt_clear_source, L.rgc_ndt_clear_target, L.rgc_ndt_swap_source_and_target):
        f.argtypes = [vp]
    L.rgc_ndt_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.rgc_ndt_compute_error.argtypes = [vp, dp, dp]
    L.rgc_ndt_num_correspondences.argtypes = [vp, ip]
    L.rgc_ndt_align.argtypes = [vp, fp, fp, dp, ip, ip, ip]
    L.rgc_ndt_get_voxels.argtypes = [vp, C.c_int, C.c_int, ip, ip, dp, dp, ip]
    L.rgc_ndt_get_raw_covariances.argtypes = [vp, C.c_int, C.c_int, dp, ip]
    L.rgc_gicp_set_max_correspondence_distance.argtypes = [vp, C.c_double]
    L.rgc_gicp_get_max_correspondence_distance.argtypes = [vp, dp]
    L.rgc_gicp_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.rgc_gicp_compute_error.argtypes = [vp, dp, dp]
    L.rgc_gicp_num_correspondences.argtypes = [vp, ip]
    L.rgc_gicp_get_correspondences.argtypes = [vp, ip, fp]
    L.rgc_gicp_align.argtypes = [vp, fp, fp, dp, dp, ip, ip, ip]
    L.rgc_gicpst_reset.argtypes = [vp]
    L.rgc_gicpst_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.rgc_gicpst_compute_error.argtypes = [vp, dp, dp]
    L.rgc_gicpst_num_correspondences.argtypes = [vp, ip]
    L.rgc_gicpst_num_searched.argtypes = [vp, ip]
    L.rgc_gicpst_get_correspondences.argtypes = [vp, ip, fp, fp, ip]
    L.rgc_gicpst_align.argtypes = [vp, fp, fp, dp, dp, ip, ip, ip]
    L.rgc_default_gicp_mp_params.argtypes = [C.POINTER(GicpMpParams)]
    L.rgc_default_gicp_mp_params.restype = None
    L.rgc_gicpmp_set_params.argtypes = [vp, C.POINTER(GicpMpParams)]
    L.rgc_gicpmp_get_params.argtypes = [vp, C.POINTER(GicpMpParams)]
    L.rgc_gicpmp_linearize.argtypes = [vp, dp, dp, dp, dp]
    L.rgc_gicpmp_num_correspondences.argtypes = [vp, ip, C.POINTER(C.c_longlong)]
    L.rgc_gicpmp_num_candidates.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.rgc_gicpmp_get_merged.argtypes = [vp, ip, dp, dp, dp]
    L.rgc_gicpmp_get_neighbors.argtypes = [vp, ip, ip, fp, C.c_int, C.POINTER(C.c_longlong)]
    L.rgc_gicpmp_align.argtypes = [vp, fp, fp, dp, dp, ip, ip, ip]
    L.rgc_search_set_cloud.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double]
    L.rgc_search_clear.argtypes = [vp]
    L.rgc_search_get_info.argtypes = [vp, C.POINTER(SearchInfo)]
    L.rgc_search_sort_window.argtypes = []
    L.rgc_search_knn.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.rgc_search_radius.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp, C.c_longlong, C.POINTER(C.c_longlong)]
    L.rgc_outlier_statistical.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, vp, ip]
    L.rgc_outlier_radius.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp, ip]
    L.rgc_outlier_get_info.argtypes = [vp, C.POINTER(OutlierInfo)]
    L.rgc_outlier_set_cell.argtypes = [vp, C.c_double]
    L.rgc_cluster_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, vp, vp, vp, ip]
    L.rgc_cluster_get_info.argtypes = [vp, C.POINTER(ClusterInfo)]
    L.rgc_cluster_set_cell.argtypes = [vp, C.c_double]
    L.rgc_default_plane_params.argtypes = [C.POINTER(PlaneParams)]
    L.rgc_default_plane_params.restype = None
    L.rgc_plane_segment.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PlaneParams), vp, C.c_int, C.c_int, vp, vp, vp, vp, ip]
    L.rgc_plane_get_info.argtypes = [vp, C.POINTER(PlaneInfo)]
    L.rgc_plane_set_batch.argtypes = [vp, C.c_int]
    L.rgc_plane_sample.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, ip]
    L.rgc_default_normal_params.argtypes = [C.POINTER(NormalParams)]
    L.rgc_default_normal_params.restype = None
    L.rgc_normal_estimate.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(NormalParams), vp, vp, vp, vp, ip]
    L.rgc_normal_get_info.argtypes = [vp, C.POINTER(NormalInfo)]
    L.rgc_normal_set_cell.argtypes = [vp, C.c_double]
    L.rgc_default_fpfh_params.argtypes = [C.POINTER(FpfhParams)]
    L.rgc_default_fpfh_params.restype = None
    L.rgc_fpfh_estimate.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.POINTER(FpfhParams), vp, vp, vp, vp, ip]
    L.rgc_fpfh_get_info.argtypes = [vp, C.POINTER(FpfhInfo)]
    L.rgc_fpfh_set_cell.argtypes = [vp, C.c_double]
    L.rgc_profile_enable.argtypes = [vp, C.c_int]
    L.rgc_profile_select.argtypes = [vp, C.c_uint]
    L.rgc_profile_reset.argtypes = [vp]
    L.rgc_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), dp, C.POINTER(C.c_longlong)]
    L.rgc_profile_name.argtypes = [C.c_int]
    L.rgc_profile_name.restype = C.c_char_p
    _lib = L
    return L


def default_params(**kw) -> Params:
    p = Params()
    load().rgc_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p
