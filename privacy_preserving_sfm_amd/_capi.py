"""ctypes binding of include/ppsfm_hip.h (libppsfm_hip.so, gfx950).

There is deliberately NO fallback: if the HIP library cannot be built/loaded the import of any
compute entry point raises, and every compute call needs a GPU.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
c_u16p = C.POINTER(C.c_uint16)
c_u32p = C.POINTER(C.c_uint32)

PP_OK, PP_ERR_INVALID, PP_ERR_HIP, PP_ERR_NUMERIC, PP_ERR_NOMEM, PP_ERR_INTERNAL = 0, -1, -2, -3, -4, -5
CAM_STRIDE = 12
BA_T_NAMES = ("eval", "reduce", "schur", "cholesky", "backsub", "update_cost")


class PPError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ppsfm_hip error %d: %s" % (code, msg))
        self.code = code


LINEAR_SOLVER_AUTO, LINEAR_SOLVER_DIRECT, LINEAR_SOLVER_ITERATIVE_SCHUR = 0, 1, 2      # PP_LINEAR_SOLVER_*


class BAProblemDesc(C.Structure):
    _fields_ = [("num_poses", C.c_int32), ("num_points", C.c_int32), ("num_cameras", C.c_int32), ("loss_type", C.c_int32),
                ("num_obs", C.c_int64), ("loss_scale", C.c_double),
                ("lines", c_dp), ("obs_pose", c_ip), ("obs_point", c_ip), ("pose_camera", c_ip), ("camera_model", c_ip),
                ("pose_const", c_u8p), ("tvec_const_mask", c_u8p), ("point_const", c_u8p), ("camera_const_mask", c_u16p),
                ("linear_solver", C.c_int32), ("ordering", C.c_int32), ("covisibility", c_u8p)]


ORDERING_DEFAULT, ORDERING_NATURAL, ORDERING_AUTO = 0, 1, 2      # PP_ORDERING_* (0 and 1: the caller's order)


class BAOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int32), ("max_num_consecutive_invalid_steps", C.c_int32),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("jacobi_scaling", C.c_int32), ("phase_timings", C.c_int32),
                ("max_linear_solver_iterations", C.c_int32), ("reserved_", C.c_int32), ("eta", C.c_double),
                ("iteration_callback", C.c_void_p), ("iteration_callback_ctx", C.c_void_p)]


class BAIterationSummary(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("step_is_successful", C.c_int32), ("cost", C.c_double), ("cost_change", C.c_double),
                ("gradient_max_norm", C.c_double), ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("trust_region_radius", C.c_double)]


ITERATION_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(BAIterationSummary))
SOLVER_CONTINUE, SOLVER_ABORT, SOLVER_TERMINATE_SUCCESSFULLY = 0, 1, 2
TERM_CONVERGENCE, TERM_NO_CONVERGENCE, TERM_FAILURE, TERM_USER_SUCCESS, TERM_USER_FAILURE = 0, 1, 2, 3, 4


class BASummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("termination", C.c_int32), ("num_iterations", C.c_int32),
                ("num_residuals", C.c_int32), ("num_effective_parameters", C.c_int32),
                ("total_time_s", C.c_double), ("device_time_s", C.c_double),
                ("linear_solver", C.c_int32), ("cholesky_fallbacks", C.c_int32), ("linear_solver_iterations", C.c_int32),
                ("reserved_", C.c_int32)]


class BACovarianceInfo(C.Structure):
    _fields_ = [("n", C.c_int32), ("path", C.c_int32), ("device_ms", C.c_double), ("reserved", C.c_double * 2)]


class CovBlock(C.Structure):
    """pp_cov_block: one requested pair of parameter blocks of pp_ba_covariance_blocks"""
    _fields_ = [("kind_a", C.c_int32), ("index_a", C.c_int32), ("kind_b", C.c_int32), ("index_b", C.c_int32)]


COV_POSE, COV_INTRINSICS, COV_POINT = 0, 1, 2
COV_WIDTH = {COV_POSE: 6, COV_INTRINSICS: 12, COV_POINT: 3}


class RansacOptions(C.Structure):
    _fields_ = [("max_error", C.c_double), ("min_inlier_ratio", C.c_double), ("confidence", C.c_double),
                ("dyn_num_trials_multiplier", C.c_double), ("min_num_trials", C.c_uint64), ("max_num_trials", C.c_uint64),
                ("seed", C.c_uint32), ("chunk_trials", C.c_uint32)]


class RansacReport(C.Structure):
    _fields_ = [("success", C.c_int32), ("best_model_index", C.c_int32), ("num_trials", C.c_uint64), ("num_inliers", C.c_uint64),
                ("residual_sum", C.c_double), ("model", C.c_double * 12), ("best_trial", C.c_int64),
                ("hypotheses_evaluated", C.c_uint64), ("models_scored", C.c_uint64),
                ("device_time_s", C.c_double), ("total_time_s", C.c_double)]


class TriangulationOptions(C.Structure):
    _fields_ = [("min_tri_angle", C.c_double), ("residual_type", C.c_int32), ("reserved", C.c_int32), ("ransac", RansacOptions)]


class FilterOptions(C.Structure):
    _fields_ = [("max_reproj_error", C.c_double), ("min_tri_angle_deg", C.c_double)]


class FilterReport(C.Structure):
    _fields_ = [("num_filtered", C.c_int64), ("num_points_deleted", C.c_int64), ("num_observations_deleted", C.c_int64)]


class TracksDesc(C.Structure):
    _fields_ = [("num_images", C.c_int32), ("num_cameras", C.c_int32), ("num_points", C.c_int32), ("reserved_", C.c_int32),
                ("num_lines", C.c_int64), ("num_corrs", C.c_int64),
                ("poses", c_dp), ("pose_camera", c_ip), ("camera_model", c_ip), ("intr", c_dp), ("cam_size", c_ip),
                ("camera_skip", c_u8p), ("image_registered", c_u8p), ("lines", c_dp), ("line_image", c_ip), ("line_point", c_ip),
                ("corr_start", c_ip), ("corr_line", c_ip), ("points", c_dp), ("track_start", c_ip), ("track_line", c_ip)]


class TracksOptions(C.Structure):
    _fields_ = [("merge_max_reproj_error", C.c_double), ("complete_max_reproj_error", C.c_double),
                ("complete_max_transitivity", C.c_int32), ("reserved_", C.c_int32)]


class TracksReport(C.Structure):
    _fields_ = [("num_changed", C.c_int64), ("num_entries", C.c_int64), ("candidates_evaluated", C.c_int64),
                ("conflict_replays", C.c_int32), ("overflow_points", C.c_int32), ("fresh_pair_launches", C.c_int32),
                ("second_launches", C.c_int32), ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class TracksImageOptions(C.Structure):
    _fields_ = [("create_max_angle_error", C.c_double), ("continue_max_angle_error", C.c_double), ("complete_max_reproj_error", C.c_double),
                ("min_angle", C.c_double), ("max_transitivity", C.c_int32), ("complete_max_transitivity", C.c_int32),
                ("ignore_two_view_tracks", C.c_int32), ("reserved_", C.c_int32)]


class TracksImageReport(C.Structure):
    _fields_ = [("num_changed", C.c_int64), ("num_entries", C.c_int64), ("ransac_trials", C.c_int64), ("points_created", C.c_int32),
                ("lines_continued", C.c_int32), ("lines_redone", C.c_int32), ("fresh_launches", C.c_int32),
                ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class LocalBundleOptions(C.Structure):
    _fields_ = [("local_ba_num_images", C.c_int32), ("reserved_", C.c_int32), ("local_ba_min_tri_angle", C.c_double)]


class LocalBundleReport(C.Structure):
    _fields_ = [("num_points3D", C.c_int32), ("num_overlapping", C.c_int32), ("num_selected", C.c_int32), ("angles_computed", C.c_int32),
                ("angles_used", C.c_int32), ("threshold_level", C.c_int32), ("filled", C.c_int32), ("reserved_", C.c_int32),
                ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class NextImageOptions(C.Structure):
    _fields_ = [("abs_pose_min_num_inliers", C.c_int32), ("max_reg_trials", C.c_int32), ("image_selection_method", C.c_int32), ("reserved_", C.c_int32)]


class NextImageReport(C.Structure):
    _fields_ = [("num_ranked", C.c_int32), ("num_first_bucket", C.c_int32), ("num_unregistered", C.c_int32), ("reserved_", C.c_int32),
                ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


REG_OK, REG_FEW_VISIBLE, REG_FEW_CORRS, REG_NO_INLIERS, REG_ALIGNED, REG_NAN, REG_FEW_INLIERS = range(7)      # PP_REG_*


class ImagePoseReport(C.Structure):
    _fields_ = [("failure", C.c_int32), ("num_visible", C.c_int32), ("num_corrs", C.c_int64), ("num_trials", C.c_uint64), ("num_inliers", C.c_int64),
                ("num_aligned_inliers", C.c_int32), ("reserved_", C.c_int32), ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class TracksFilterReport(C.Structure):
    _fields_ = [("num_filtered", C.c_int64), ("num_points_deleted", C.c_int64), ("num_observations_deleted", C.c_int64), ("num_entries", C.c_int64),
                ("points_tested", C.c_int32), ("images_filtered", C.c_int32), ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class InitSetsOptions(C.Structure):
    _fields_ = [("min_num_aligned_tracks", C.c_int32), ("min_num_random_tracks", C.c_int32), ("max_num_sets", C.c_int32), ("reserved_", C.c_int32),
                ("max_candidates", C.c_int64)]


class InitSetsReport(C.Structure):
    _fields_ = [("num_candidates", C.c_int64), ("num_aligned_tracks", C.c_int64), ("num_random_tracks", C.c_int64), ("num_track_entries", C.c_int64),
                ("num_aligned_sets", C.c_int32), ("num_random_sets", C.c_int32), ("num_qualified", C.c_int32), ("num_returned", C.c_int32),
                ("num_work_lines", C.c_int32), ("overflow_lines", C.c_int32), ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class BundleConfig(C.Structure):
    _fields_ = [("image_flags", c_u8p), ("tvec_const_mask", c_u8p), ("camera_const", c_u8p), ("camera_subset_mask", c_u16p),
                ("variable_points", c_ip), ("constant_points", c_ip), ("num_variable_points", C.c_int32), ("num_constant_points", C.c_int32)]


class BundleSetupReport(C.Structure):
    _fields_ = [("num_obs", C.c_int64), ("num_config_obs", C.c_int64), ("num_poses", C.c_int32), ("num_config_poses", C.c_int32),
                ("num_points", C.c_int32), ("num_cameras", C.c_int32), ("bad_line", C.c_int64),
                ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


PP_BUNDLE_IMAGE, PP_BUNDLE_CONST_POSE = 1, 2


class SiftMatchOptions(C.Structure):
    _fields_ = [("max_ratio", C.c_double), ("max_distance", C.c_double), ("cross_check", C.c_int32), ("min_num_matches", C.c_int32),
                ("workspace_bytes", C.c_int64)]


class SiftMatchReport(C.Structure):
    _fields_ = [("num_matches", C.c_int64), ("num_pairs_emptied", C.c_int32), ("num_batches", C.c_int32), ("device_ms", C.c_double), ("total_ms", C.c_double)]


class CorrGraphReport(C.Structure):
    _fields_ = [("num_pairs_used", C.c_int64), ("num_pairs_ignored", C.c_int64), ("num_matches_in", C.c_int64), ("num_matches_accepted", C.c_int64),
                ("num_matches_bad_index", C.c_int64), ("num_matches_duplicate", C.c_int64), ("num_pairs_replayed", C.c_int64),
                ("device_ms", C.c_double), ("replay_ms", C.c_double), ("total_ms", C.c_double)]


class LineFeaturesDesc(C.Structure):
    _fields_ = [("num_images", C.c_int32), ("num_cameras", C.c_int32), ("image_ids", c_ip), ("kp_start", C.POINTER(C.c_int64)),
                ("keypoints", C.POINTER(C.c_float)), ("image_camera", c_ip), ("camera_model", c_ip), ("intr", c_dp), ("has_gravity", c_u8p),
                ("gravity", c_dp)]


class LineFeaturesOptions(C.Structure):
    _fields_ = [("aligned_line_ratio", C.c_double), ("seed", C.c_uint64)]


class LineFeaturesReport(C.Structure):
    _fields_ = [("num_lines", C.c_int64), ("num_aligned", C.c_int64), ("num_images_without_gravity", C.c_int64), ("num_degenerate", C.c_int64),
                ("num_newton_exhausted", C.c_int64), ("device_ms", C.c_double)]


class PairsReport(C.Structure):
    _fields_ = [("num_pairs", C.c_int64), ("num_candidates", C.c_int64), ("device_ms", C.c_double), ("total_ms", C.c_double)]


SIFT_MAX_OCTAVES = 32      # PP_SIFT_MAX_OCTAVES
SIFT_L1_ROOT, SIFT_L2 = 0, 1
SIFT_STAGE_GAUSSIAN, SIFT_STAGE_DOG, SIFT_STAGE_GRADIENT = 0, 1, 2
SIFT_PHASES = ("pyramid", "detection", "gradient", "orientation", "descriptor")


class SiftExtractOptions(C.Structure):
    _fields_ = [("max_num_features", C.c_int32), ("first_octave", C.c_int32), ("num_octaves", C.c_int32), ("octave_resolution", C.c_int32),
                ("peak_threshold", C.c_double), ("edge_threshold", C.c_double), ("max_num_orientations", C.c_int32), ("upright", C.c_int32),
                ("normalization", C.c_int32), ("phase_timings", C.c_int32)]


class SiftExtractReport(C.Structure):
    _fields_ = [("num_octaves", C.c_int32), ("num_levels", C.c_int32), ("first_level_to_keep", C.c_int32), ("reserved_", C.c_int32),
                ("num_keypoints", C.c_int64), ("num_features_found", C.c_int64), ("num_features", C.c_int64), ("num_two_orientations", C.c_int64),
                ("num_moved", C.c_int64), ("num_rejected_peak", C.c_int64), ("num_rejected_edge", C.c_int64), ("num_rejected_offset", C.c_int64),
                ("num_rejected_bounds", C.c_int64), ("num_windows_cut", C.c_int64), ("num_descriptors_skipped", C.c_int64),
                ("octave_width", C.c_int32 * SIFT_MAX_OCTAVES), ("octave_height", C.c_int32 * SIFT_MAX_OCTAVES),
                ("octave_candidates", C.c_int32 * SIFT_MAX_OCTAVES), ("octave_keypoints", C.c_int32 * SIFT_MAX_OCTAVES),
                ("phase_ms", C.c_double * 5), ("device_ms", C.c_double), ("total_ms", C.c_double)]


class SiftBatchImage(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("grey", C.POINTER(C.c_uint8))]


class SiftBatchReport(C.Structure):
    _fields_ = [("num_images", C.c_int32), ("num_sub_batches", C.c_int32), ("num_features", C.c_int64), ("workspace_bytes", C.c_int64),
                ("phase_ms", C.c_double * 5), ("device_ms", C.c_double), ("total_ms", C.c_double)]


class LoMsacOptions(C.Structure):
    _fields_ = [("min_num_iterations", C.c_uint32), ("max_num_iterations", C.c_uint32), ("success_probability", C.c_double),
                ("squared_inlier_threshold", C.c_double), ("random_seed", C.c_uint32), ("num_lo_steps", C.c_int32),
                ("threshold_multiplier", C.c_double), ("num_lsq_iterations", C.c_int32), ("min_sample_multiplicator", C.c_int32),
                ("non_min_sample_multiplier", C.c_int32), ("lo_starting_iterations", C.c_uint32), ("final_least_squares", C.c_int32),
                ("chunk_iterations", C.c_uint32)]


class LoMsacReport(C.Structure):
    _fields_ = [("num_iterations", C.c_uint32), ("best_num_inliers", C.c_int32), ("best_model_score", C.c_double),
                ("inlier_ratio", C.c_double), ("number_lo_iterations", C.c_int32), ("num_inlier_indices", C.c_int32),
                ("hypotheses_evaluated", C.c_uint64), ("device_time_s", C.c_double), ("total_time_s", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)

_EXPORTS = [
    "pp_last_error", "pp_device_count", "pp_debug_raise", "pp_debug_exclusive_scan", "pp_camera_num_params", "pp_camera_image_to_world_threshold",
    "pp_camera_image_to_world", "pp_camera_world_to_image",
    "pp_ba_options_default", "pp_ba_create", "pp_ba_destroy", "pp_ba_set_parameters", "pp_ba_get_parameters",
    "pp_ba_eval", "pp_ba_eval_host_view", "pp_ba_eval_device", "pp_ba_solve", "pp_ba_get_trace", "pp_ba_get_structure", "pp_ba_get_intrinsics_layout", "pp_ba_plan_ordering", "pp_ba_pair_lists_host", "pp_ba_covisibility", "pp_ba_get_create_profile", "pp_ba_reduced_system", "pp_ba_covariance", "pp_ba_covariance_blocks", "pp_ba_set_allreduce", "pp_ba_set_communicator", "pp_comm_unique_id", "pp_comm_create", "pp_comm_destroy",
    "pp_comm_allreduce",
    "pp_ba_get_timings", "pp_pool_trim", "pp_pool_stats", "pp_dense_cholesky_solve", "pp_cholesky_task_list", "pp_cholesky_task_list_sparse", "pp_cholesky_task_plan",
    "pp_pose_create", "pp_pose_destroy", "pp_pose_residuals", "pp_pose_score", "pp_pose_support_sequential",
    "pp_pose_p6l_batch", "pp_re3q3_batch", "pp_ransac_options_default", "pp_pose_ransac", "pp_pose_hypotheses", "pp_pose_last_scores",
    "pp_sampler_draw", "pp_ransac_compute_num_trials",
    "pp_lomsac_options_default", "pp_planar_create", "pp_planar_destroy", "pp_planar_solve_batch", "pp_planar_score",
    "pp_planar_evaluate", "pp_planar_lomsac", "pp_fourview2d_create", "pp_fourview2d_destroy", "pp_fourview2d_score",
    "pp_triangulate_tracks", "pp_ba_filter_points", "pp_ba_filter_negative_depth", "pp_pose2d_create", "pp_pose2d_destroy", "pp_pose2d_solve_batch", "pp_pose2d_score", "pp_pose2d_evaluate", "pp_pose2d_lomsac",
    "pp_tracks_options_default", "pp_tracks_create", "pp_tracks_destroy", "pp_tracks_complete", "pp_tracks_merge", "pp_tracks_get_state",
    "pp_tracks_image_options_default", "pp_tracks_triangulate_image", "pp_tracks_complete_image",
    "pp_local_bundle_options_default", "pp_tracks_find_local_bundle", "pp_tracks_update",
    "pp_next_image_options_default", "pp_tracks_find_next_images", "pp_tracks_estimate_image_pose", "pp_tracks_register_image",
    "pp_tracks_filter_points", "pp_tracks_filter_negative_depth", "pp_tracks_filter_images",
    "pp_init_sets_options_default", "pp_tracks_find_initial_sets", "pp_tracks_bundle_setup",
    "pp_sift_match_options_default", "pp_sift_create", "pp_sift_destroy", "pp_sift_match_pairs", "pp_sift_top2", "pp_sift_match_thresholds",
    "pp_sift_get_descriptors",
    "pp_corr_graph_create", "pp_corr_graph_destroy", "pp_corr_graph_build", "pp_corr_graph_num_entries", "pp_corr_graph_get", "pp_corr_graph_pair_counts",
    "pp_line_features_options_default", "pp_line_features_from_keypoints",
    "pp_pairs_create", "pp_pairs_destroy", "pp_pairs_spatial", "pp_pairs_transitive", "pp_pairs_num", "pp_pairs_get",
    "pp_sift_extract_options_default", "pp_sift_extractor_create", "pp_sift_extractor_destroy", "pp_sift_extract", "pp_sift_extract_stage",
    "pp_sift_extract_candidates", "pp_sift_extract_features", "pp_sift_extract_batch", "pp_sift_extract_batch_features",
    "pp_sift_extract_to_matcher",
    "pp_fourview2d_evaluate", "pp_fourview2d_evaluate_points", "pp_fourview2d_default_frames", "pp_fourview2d_minimal_batch", "pp_fourview2d_nonminimal_batch", "pp_fourview2d_least_squares", "pp_fourview2d_lomsac",
]

_lib = None


def exported_symbols():
    """Every symbol include/ppsfm_hip.h declares."""
    return list(_EXPORTS)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if _build.is_stale():
        _build.build_library()
    if not os.path.exists(_build.LIB):
        raise ImportError("libppsfm_hip.so is missing and could not be built (hipcc required); "
                          "there is no CPU fallback for the product path")
    L = C.CDLL(_build.LIB)
    L.pp_last_error.restype = C.c_char_p
    L.pp_ransac_compute_num_trials.restype = C.c_uint64
    L.pp_ransac_compute_num_trials.argtypes = [C.c_uint64, C.c_uint64, C.c_double, C.c_double]
    L.pp_ba_create.argtypes = [C.POINTER(BAProblemDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.pp_ba_destroy.argtypes = [C.c_void_p]
    L.pp_ba_set_parameters.argtypes = [C.c_void_p, c_dp, c_dp, c_dp]
    L.pp_ba_get_parameters.argtypes = [C.c_void_p, c_dp, c_dp, c_dp]
    L.pp_ba_eval.argtypes = [C.c_void_p, C.c_int, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp]
    L.pp_ba_eval_host_view.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(c_dp), C.POINTER(c_dp), C.POINTER(c_dp), C.POINTER(c_dp), c_dp]
    L.pp_ba_eval_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.pp_ba_solve.argtypes = [C.c_void_p, C.POINTER(BAOptions), C.POINTER(BASummary)]
    L.pp_ba_get_trace.argtypes = [C.c_void_p, c_dp, C.c_int32, c_ip]
    L.pp_ba_get_structure.argtypes = [C.c_void_p, c_ip]
    L.pp_ba_get_intrinsics_layout.argtypes = [C.c_void_p, c_ip]
    L.pp_ba_plan_ordering.argtypes = [C.POINTER(BAProblemDesc), c_ip, c_ip]
    L.pp_ba_pair_lists_host.argtypes = [C.POINTER(BAProblemDesc), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), c_ip, c_ip, c_ip, C.c_int64, C.c_int64]
    L.pp_ba_covisibility.argtypes = [C.POINTER(BAProblemDesc), c_u8p]
    L.pp_ba_get_create_profile.argtypes = [C.c_void_p, c_dp]
    L.pp_ba_reduced_system.argtypes = [C.c_void_p, C.POINTER(BAOptions), C.c_double, c_ip, c_dp, c_dp, C.c_int64]
    L.pp_ba_covariance.argtypes = [C.c_void_p, C.POINTER(BAOptions), C.c_int32, c_ip, c_ip, c_dp, C.c_int32, c_ip, c_dp, C.POINTER(BACovarianceInfo)]
    L.pp_ba_covariance_blocks.argtypes = [C.c_void_p, C.POINTER(BAOptions), C.c_int64, C.POINTER(CovBlock), c_dp, C.c_int64, C.POINTER(BACovarianceInfo)]
    L.pp_ba_set_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    L.pp_ba_set_communicator.argtypes = [C.c_void_p, C.c_void_p]
    L.pp_comm_unique_id.argtypes = [c_u8p]
    L.pp_comm_create.argtypes = [c_u8p, C.c_int32, C.c_int32, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_comm_destroy.argtypes = [C.c_void_p]
    L.pp_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    L.pp_ba_get_timings.argtypes = [C.c_void_p, c_dp, c_ip]
    L.pp_pool_stats.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pp_dense_cholesky_solve.argtypes = [C.c_int32, c_dp, c_dp, c_dp, C.c_int, C.c_int32, C.POINTER(C.c_float)]
    L.pp_cholesky_task_list.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
    L.pp_cholesky_task_list_sparse.argtypes = [C.c_int32, c_u8p, c_u8p, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)]
    L.pp_cholesky_task_plan.argtypes = [C.c_int32, c_u8p, C.c_int32, c_u8p, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.pp_pose_create.argtypes = [C.c_int32, c_dp, c_dp, c_u8p, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_pose_destroy.argtypes = [C.c_void_p]
    L.pp_pose_residuals.argtypes = [C.c_void_p, C.c_int32, c_dp, c_dp]
    L.pp_pose_score.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_double, c_u32p, c_dp]
    L.pp_pose_support_sequential.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_double, c_u32p, c_dp]
    L.pp_pose_p6l_batch.argtypes = [C.c_void_p, C.c_int64, c_u32p, c_dp, c_ip]
    L.pp_re3q3_batch.argtypes = [C.c_int64, c_dp, c_dp, c_ip, C.c_int]
    L.pp_pose_ransac.argtypes = [C.c_void_p, C.POINTER(RansacOptions), C.POINTER(RansacReport), c_u8p]
    L.pp_pose_hypotheses.argtypes = [C.c_void_p, C.c_int64, c_u32p, C.c_uint32, C.c_double, C.POINTER(RansacReport)]
    L.pp_pose_last_scores.argtypes = [C.c_void_p, C.c_int64, c_ip, c_u32p, c_dp]
    L.pp_debug_raise.argtypes = [C.c_int]
    L.pp_debug_exclusive_scan.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pp_sampler_draw.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int64, c_u32p]
    L.pp_planar_create.argtypes = [C.c_int32, c_dp, c_dp, c_dp, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_planar_destroy.argtypes = [C.c_void_p]
    L.pp_planar_solve_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_ip, c_dp]
    L.pp_planar_score.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_double, c_dp, c_ip]
    L.pp_planar_evaluate.argtypes = [C.c_void_p, c_dp, c_dp, c_dp, c_dp]
    L.pp_planar_lomsac.argtypes = [C.c_void_p, C.POINTER(LoMsacOptions), C.POINTER(LoMsacReport), c_dp, c_dp, c_ip]
    L.pp_triangulate_tracks.argtypes = [C.c_int, C.c_int32, c_ip, c_dp, c_ip, C.c_int32, c_dp, c_dp, c_ip, C.c_int32, c_ip, c_dp, c_ip,
                                        C.POINTER(TriangulationOptions), c_u8p, c_dp, c_u8p, c_ip, C.POINTER(C.c_float)]
    L.pp_ba_filter_points.argtypes = [C.c_void_p, C.POINTER(FilterOptions), c_u8p, c_ip, c_u8p, c_u8p, c_u8p, c_dp, C.POINTER(FilterReport)]
    L.pp_ba_filter_negative_depth.argtypes = [C.c_void_p, c_u8p, C.POINTER(C.c_int64)]
    L.pp_pose2d_create.argtypes = [C.c_int32, c_dp, c_dp, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_pose2d_destroy.argtypes = [C.c_void_p]
    L.pp_pose2d_solve_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_ip, c_dp]
    L.pp_pose2d_score.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_double, c_dp, c_ip]
    L.pp_pose2d_evaluate.argtypes = [C.c_void_p, c_dp, c_dp]
    L.pp_pose2d_lomsac.argtypes = [C.c_void_p, C.POINTER(LoMsacOptions), C.POINTER(LoMsacReport), c_dp, c_ip]
    L.pp_fourview2d_create.argtypes = [C.c_int32, c_dp, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_fourview2d_destroy.argtypes = [C.c_void_p]
    L.pp_fourview2d_score.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_double, c_dp, c_ip]
    L.pp_fourview2d_evaluate.argtypes = [C.c_void_p, c_dp, c_dp, c_dp]
    L.pp_fourview2d_evaluate_points.argtypes = [C.c_void_p, c_dp, c_dp, c_dp]
    L.pp_fourview2d_default_frames.argtypes = [c_dp]
    L.pp_fourview2d_minimal_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_ip, c_dp, c_dp, c_ip]
    L.pp_fourview2d_nonminimal_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int32, c_ip, c_dp, C.c_double, c_dp, c_dp, c_ip]
    L.pp_fourview2d_least_squares.argtypes = [C.c_void_p, C.c_int32, c_ip, c_dp, c_dp]
    L.pp_fourview2d_lomsac.argtypes = [C.c_void_p, C.POINTER(LoMsacOptions), c_dp, C.POINTER(LoMsacReport), c_dp, c_dp, c_ip]
    L.pp_tracks_options_default.argtypes = [C.POINTER(TracksOptions)]
    L.pp_tracks_create.argtypes = [C.POINTER(TracksDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.pp_tracks_destroy.argtypes = [C.c_void_p]
    L.pp_tracks_complete.argtypes = [C.c_void_p, C.POINTER(TracksOptions), c_u8p, C.POINTER(TracksReport), c_ip, c_ip, C.c_int64]
    L.pp_tracks_merge.argtypes = [C.c_void_p, C.POINTER(TracksOptions), c_u8p, C.POINTER(TracksReport), c_ip, c_ip, c_ip, C.c_int64]
    L.pp_tracks_get_state.argtypes = [C.c_void_p, c_ip, C.POINTER(C.c_int64), c_ip, c_dp, c_u8p, c_ip, c_ip, C.c_int32, C.c_int64]
    L.pp_tracks_image_options_default.argtypes = [C.POINTER(TracksImageOptions)]
    L.pp_tracks_triangulate_image.argtypes = [C.c_void_p, C.POINTER(TracksImageOptions), C.c_int32, c_u8p, C.POINTER(TracksImageReport), c_ip, c_ip, C.c_int64]
    L.pp_tracks_complete_image.argtypes = [C.c_void_p, C.POINTER(TracksImageOptions), C.c_int32, C.POINTER(TracksImageReport), c_ip, c_ip, C.c_int64]
    L.pp_local_bundle_options_default.argtypes = [C.POINTER(LocalBundleOptions)]
    L.pp_tracks_find_local_bundle.argtypes = [C.c_void_p, C.POINTER(LocalBundleOptions), C.c_int32, C.POINTER(LocalBundleReport), c_ip, C.c_int32, c_ip, c_ip, c_dp]
    L.pp_tracks_update.argtypes = [C.c_void_p, C.c_int32, c_ip, c_dp, C.c_int32, c_ip, c_dp, c_dp, c_u8p]
    L.pp_next_image_options_default.argtypes = [C.POINTER(NextImageOptions)]
    L.pp_tracks_find_next_images.argtypes = [C.c_void_p, C.POINTER(NextImageOptions), c_ip, c_u8p, C.POINTER(NextImageReport), c_ip, C.c_int32, c_ip, c_ip]
    L.pp_tracks_estimate_image_pose.argtypes = [C.c_void_p, C.POINTER(NextImageOptions), C.POINTER(RansacOptions), C.c_int32, c_u8p, C.POINTER(ImagePoseReport),
                                                c_dp, c_ip, c_ip, c_u8p, C.c_int64]
    L.pp_tracks_register_image.argtypes = [C.c_void_p, C.c_int32, c_dp, C.c_int64, c_ip, c_ip, c_u8p, C.POINTER(C.c_int64), c_ip, c_ip, C.c_int64]
    L.pp_tracks_filter_points.argtypes = [C.c_void_p, C.POINTER(FilterOptions), c_u8p, c_u8p, c_u8p, C.POINTER(TracksFilterReport), c_ip, c_ip, C.c_int64, c_dp]
    L.pp_tracks_filter_negative_depth.argtypes = [C.c_void_p, c_ip, C.c_int32, C.POINTER(TracksFilterReport), c_ip, c_ip, C.c_int64]
    L.pp_tracks_filter_images.argtypes = [C.c_void_p, c_ip, C.c_int32, c_ip, C.POINTER(TracksFilterReport), c_ip, c_ip, C.c_int64]
    L.pp_init_sets_options_default.argtypes = [C.POINTER(InitSetsOptions)]
    L.pp_tracks_find_initial_sets.argtypes = [C.c_void_p, C.POINTER(InitSetsOptions), c_u8p, c_u8p, c_ip, C.c_int32, C.POINTER(InitSetsReport), c_ip, c_ip, c_ip,
                                              C.POINTER(C.c_int64), c_ip, C.c_int64]
    L.pp_tracks_bundle_setup.argtypes = [C.c_void_p, C.POINTER(BundleConfig), C.POINTER(BundleSetupReport), c_dp, c_ip, c_ip, c_ip, C.c_int64,
                                         c_ip, c_u8p, c_u8p, c_ip, c_ip, c_u8p, c_dp, C.c_int32, c_ip, c_u16p]
    L.pp_sift_match_options_default.argtypes = [C.POINTER(SiftMatchOptions)]
    L.pp_sift_match_options_default.restype = None
    L.pp_sift_create.argtypes = [C.c_int32, C.POINTER(C.c_int64), c_u8p, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_sift_destroy.argtypes = [C.c_void_p]
    L.pp_sift_match_pairs.argtypes = [C.c_void_p, C.POINTER(SiftMatchOptions), C.c_int64, c_ip, C.POINTER(SiftMatchReport), C.POINTER(C.c_int64), c_ip, C.c_int64]
    L.pp_sift_top2.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_ip, c_ip, c_ip]
    L.pp_sift_match_thresholds.argtypes = [C.POINTER(SiftMatchOptions), c_ip, c_ip, C.c_int64, C.POINTER(C.c_int64)]
    L.pp_sift_get_descriptors.argtypes = [C.c_void_p, C.c_int32, c_u8p, C.c_int64, C.POINTER(C.c_int64)]
    L.pp_corr_graph_create.argtypes = [C.c_int32, c_ip, C.c_int, C.POINTER(C.c_void_p)]
    L.pp_corr_graph_destroy.argtypes = [C.c_void_p]
    L.pp_corr_graph_build.argtypes = [C.c_void_p, C.c_int32, C.c_int64, c_ip, C.POINTER(C.c_int64), c_ip, C.POINTER(CorrGraphReport)]
    L.pp_corr_graph_num_entries.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pp_corr_graph_get.argtypes = [C.c_void_p, c_ip, c_ip, C.c_int64, c_u8p, c_ip, c_ip]
    L.pp_corr_graph_pair_counts.argtypes = [C.c_void_p, c_ip]
    L.pp_camera_image_to_world_threshold.argtypes = [C.c_int, c_dp, C.c_double, c_dp]
    L.pp_camera_image_to_world.argtypes = [C.c_int, c_dp, C.c_int64, c_dp, c_dp]
    L.pp_camera_world_to_image.argtypes = [C.c_int, c_dp, C.c_int64, c_dp, c_dp]
    L.pp_line_features_options_default.argtypes = [C.POINTER(LineFeaturesOptions)]
    L.pp_line_features_options_default.restype = None
    L.pp_line_features_from_keypoints.argtypes = [C.POINTER(LineFeaturesDesc), C.POINTER(LineFeaturesOptions), C.c_int, c_dp, c_u8p, c_dp,
                                                  C.POINTER(LineFeaturesReport)]
    L.pp_pairs_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.pp_pairs_destroy.argtypes = [C.c_void_p]
    L.pp_pairs_spatial.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_int32, C.c_double, C.POINTER(PairsReport)]
    L.pp_pairs_transitive.argtypes = [C.c_void_p, C.c_int32, C.c_int64, c_ip, C.c_int64, c_ip, C.POINTER(PairsReport)]
    L.pp_pairs_num.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.pp_pairs_get.argtypes = [C.c_void_p, c_ip, C.POINTER(C.c_float), C.c_int64]
    L.pp_sift_extract_options_default.argtypes = [C.POINTER(SiftExtractOptions)]
    L.pp_sift_extract_options_default.restype = None
    L.pp_sift_extractor_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.pp_sift_extractor_destroy.argtypes = [C.c_void_p]
    L.pp_sift_extract.argtypes = [C.c_void_p, C.POINTER(SiftExtractOptions), C.c_int32, C.c_int32, c_u8p, C.POINTER(SiftExtractReport), C.c_int64,
                                  C.POINTER(C.c_float), c_u8p, C.POINTER(C.c_int64)]
    L.pp_sift_extract_stage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int64, c_ip, c_ip]
    L.pp_sift_extract_candidates.argtypes = [C.c_void_p, C.c_int32, c_ip, C.c_int64, C.POINTER(C.c_int64)]
    L.pp_sift_extract_features.argtypes = [C.c_void_p, C.POINTER(C.c_float), c_ip, c_dp, C.c_int64, C.POINTER(C.c_int64)]
    L.pp_sift_extract_batch.argtypes = [C.c_void_p, C.POINTER(SiftExtractOptions), C.c_int32, C.POINTER(SiftBatchImage), C.c_int64, C.POINTER(SiftBatchReport),
                                        C.POINTER(SiftExtractReport), C.c_int64, C.POINTER(C.c_float), c_u8p, C.POINTER(C.c_int64)]
    L.pp_sift_extract_batch_features.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float), c_ip, c_dp, C.c_int64, C.POINTER(C.c_int64)]
    L.pp_sift_extract_to_matcher.argtypes = [C.c_void_p, C.POINTER(SiftExtractOptions), C.c_int32, C.POINTER(SiftBatchImage), C.c_int64, C.POINTER(SiftBatchReport),
                                             C.POINTER(SiftExtractReport), C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise PPError(rc, lib().pp_last_error().decode(errors="replace"))


def options(struct_type, default_fn_name, **kw):
    """struct_type as its pp_*_options_default fills it, then the fields named by keyword; a name the struct does not have raises AttributeError(name)"""
    o = struct_type()
    getattr(lib(), default_fn_name)(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)
