"""ctypes binding of librspl.so (the C ABI declared in include/rspl.h).

This is the product path: every call goes to the HIP library.  There is no CPU
fallback -- if librspl.so is missing or no HIP device is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib

PKG = pathlib.Path(__file__).resolve().parent
# RSPL_LIB: another in-tree build of the same ABI (A/B timing of two builds in one GPU call)
LIB_PATH = PKG / os.environ.get("RSPL_LIB", "librspl.so")

RSPL_OK = 0
RSPL_ABI_VERSION = 2  # include/rspl.h: the struct layouts the ctypes mirrors below follow
RSPL_PREC_FP32 = 0
RSPL_PREC_FP16 = 1
RSPL_PREC_FP16X3 = 2  # SuperPoint only: split fp16 (hi + lo planes, three fp16 MFMA products per step)

BA_TRACE_W = 12  # RSPL_BA_TRACE_W
BA_TRACE_FIELDS = ("submit", "stage0", "stage1", "run0", "upload", "opt1", "opt2", "end", "slot", "grew", "iters",  # grew: rspl_ba_trace [9] flags
                   "sync")

EXPORTS = [
    "rspl_last_error", "rspl_version", "rspl_abi_version",
    "rspl_device_count", "rspl_set_device", "rspl_malloc", "rspl_free", "rspl_memcpy_h2d", "rspl_memcpy_d2h",
    "rspl_memset", "rspl_memcpy_d2d", "rspl_stream_create", "rspl_stream_create_priority", "rspl_stream_create_reserving", "rspl_stream_destroy", "rspl_stream_synchronize",
    "rspl_device_synchronize", "rspl_event_create", "rspl_event_record", "rspl_stream_wait_event",
    "rspl_event_destroy", "rspl_timer_create", "rspl_timer_record", "rspl_timer_elapsed_ms",
    "rspl_timer_destroy",
    "rspl_sp_create", "rspl_sp_infer", "rspl_sp_infer_device", "rspl_sp_debug_maps", "rspl_sp_debug_nms", "rspl_sp_debug_layer",
    "rspl_sp_debug_select",
    "rspl_sp_profile",
    "rspl_sp_stage_times", "rspl_sp_destroy",
    "rspl_sg_create", "rspl_sg_infer", "rspl_sg_infer_device", "rspl_sg_infer_device2", "rspl_sg_debug_scores", "rspl_sg_profile",
    "rspl_sg_status", "rspl_sg_debug_inject", "rspl_sg_debug_sinkhorn", "rspl_sg_debug_decode", "rspl_sg_debug_layers",
    "rspl_sg_debug_sinkhorn_plan",
    "rspl_sg_stage_times", "rspl_sg_destroy",
    "rspl_pm_match",
    "rspl_ba_create", "rspl_ba_local", "rspl_ba_submit", "rspl_ba_join", "rspl_ba_destroy", "rspl_ba_use_reserved_cus", "rspl_ba_kernel_timing",
    "rspl_ba_kernel_times", "rspl_ba_trace", "rspl_ba_set_line_jacobian", "rspl_ba_debug_stage",
    "rspl_ba_debug_chunk_plan", "rspl_ba_debug_chunk_geometry",
    "rspl_ba_debug_pair_offsets", "rspl_ba_debug_pairs", "rspl_ba_debug_final",
    "rspl_frame_create", "rspl_frame_optimize", "rspl_frame_destroy",
    "rspl_ba_set_shard", "rspl_comm_unique_id", "rspl_comm_create", "rspl_comm_allreduce_sum", "rspl_comm_destroy",
    "rspl_ba_set_comm", "rspl_group_create", "rspl_group_destroy", "rspl_ba_set_group",
    "rspl_pnp_create", "rspl_pnp_solve", "rspl_pnp_destroy", "rspl_pnp_debug_hypotheses",
    "rspl_line_extract", "rspl_lines_create", "rspl_lines_destroy", "rspl_lines_assign", "rspl_lines_match",
    "rspl_lines_stereo", "rspl_lines_stereo_device", "rspl_lines_status", "rspl_lines_detect",
    "rspl_lines_debug_canny",
    "rspl_lines_detect_device", "rspl_lines_detect_status", "rspl_lines_extract_async_device",
    "rspl_lines_debug_hysteresis", "rspl_lines_debug_chains", "rspl_lines_debug_fld_host",
    "rspl_lines_debug_fld_classes",
    "rspl_lines_debug_fld_stats", "rspl_lines_debug_fld_profile", "rspl_lines_debug_fld_stage_ms",
    "rspl_track_create", "rspl_track_destroy", "rspl_track_set_keyframe", "rspl_track_enqueue", "rspl_track_fetch",
    "rspl_track_debug_stage", "rspl_track_keyframe_table",
    "rspl_track_enable_lines", "rspl_track_set_keyframe_lines", "rspl_track_enqueue_ext", "rspl_track_fetch_ext",
    "rspl_track_debug_lines", "rspl_track_frame_lines",
    "rspl_kf_create", "rspl_kf_destroy", "rspl_kf_enqueue", "rspl_kf_fetch", "rspl_kf_triangulate",
    "rspl_map_insert_keyframe", "rspl_map_get_mapline_observers",
    "rspl_rect_build_maps", "rspl_rect_debug_fixed", "rspl_rect_debug_sizeof", "rspl_rect_debug_copy", "rspl_rect_create", "rspl_rect_destroy",
    "rspl_rect_get_maps", "rspl_rect_set_maps", "rspl_rect_enqueue_device", "rspl_rect_pair",
    "rspl_rcf_debug_sizeof", "rspl_rcf_create", "rspl_rcf_destroy", "rspl_rcf_infer", "rspl_rcf_infer_device",
    "rspl_rcf_debug_logits", "rspl_rcf_debug_tile_rows", "rspl_rcf_profile", "rspl_rcf_stage_times",
    "rspl_fm_create", "rspl_fm_destroy", "rspl_fm_solve", "rspl_fm_enqueue", "rspl_fm_fetch",
    "rspl_fm_debug_subsets", "rspl_fm_debug_seven_point", "rspl_fm_debug_hypotheses",
    "rspl_lmap_create", "rspl_lmap_destroy", "rspl_lmap_store", "rspl_lmap_store_host", "rspl_lmap_bank_size",
    "rspl_lmap_set_local", "rspl_lmap_enqueue", "rspl_lmap_fetch", "rspl_lmap_debug_points", "rspl_lmap_track_enqueue",
    "rspl_lmap_debug_search_host", "rspl_map_reference_keyframe", "rspl_map_local_mappoints",
    "rspl_lmap_global_enqueue", "rspl_lmap_global_fetch", "rspl_lmap_debug_global_host", "rspl_lmap_debug_global_plan",
    "rspl_map_good_mappoints",
    "rspl_pgo_create", "rspl_pgo_destroy", "rspl_pgo_solve", "rspl_pgo_debug_host", "rspl_pgo_debug_plan",
    "rspl_pgo_debug_system", "rspl_map_pose_graph", "rspl_map_apply_pose_graph", "rspl_map_loop_candidates",
]


class SpConfig(C.Structure):
    _fields_ = [("max_keypoints", C.c_int), ("keypoint_threshold", C.c_double), ("remove_borders", C.c_int),
                ("max_height", C.c_int), ("max_width", C.c_int), ("max_batch", C.c_int),
                ("precision", C.c_int), ("device", C.c_int)]


class SgConfig(C.Structure):
    _fields_ = [("image_width", C.c_int), ("image_height", C.c_int), ("max_keypoints", C.c_int),
                ("max_batch", C.c_int), ("sinkhorn_iterations", C.c_int), ("precision", C.c_int),
                ("device", C.c_int)]


class SgSinkhornPlan(C.Structure):
    _fields_ = [("kind", C.c_int32), ("groups", C.c_int32), ("rows_per_wave", C.c_int32), ("reserved", C.c_int32),
                ("ug_granules", C.c_uint64), ("vg_granules", C.c_uint64)]


class BaChunkPlan(C.Structure):
    _fields_ = [("nchk", C.c_int32), ("lmchunk", C.c_int32), ("dsub", C.c_int32), ("lmsub", C.c_int32),
                ("chunks", C.c_int32), ("grid", C.c_int32), ("ue_bpr", C.c_int32), ("slots", C.c_int64)]


class DMatch(C.Structure):
    _fields_ = [("query_idx", C.c_int32), ("train_idx", C.c_int32), ("distance", C.c_float)]


class BaConfig(C.Structure):
    _fields_ = [("max_poses", C.c_int), ("max_points", C.c_int), ("max_lines", C.c_int),
                ("max_edges", C.c_int), ("device", C.c_int)]


class FrameConfig(C.Structure):
    _fields_ = [("max_batch", C.c_int), ("max_edges", C.c_int), ("max_points", C.c_int), ("device", C.c_int)]


class PnpConfig(C.Structure):
    _fields_ = [("max_batch", C.c_int), ("max_points", C.c_int), ("device", C.c_int)]


class PnpProblem(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("n", C.c_int),
                ("points", C.POINTER(C.c_double)), ("keypoints", C.POINTER(C.c_double)),
                ("iterations", C.c_int), ("reprojection_error", C.c_double), ("confidence", C.c_double)]


class PnpResult(C.Structure):
    _fields_ = [("Rwc", C.c_double * 9), ("twc", C.c_double * 3), ("inlier", C.POINTER(C.c_uint8)),
                ("n_inliers", C.c_int), ("hypotheses", C.c_int)]


class FmConfig(C.Structure):
    _fields_ = [("max_batch", C.c_int), ("max_matches", C.c_int), ("max_iters", C.c_int), ("device", C.c_int)]


class FmProblem(C.Structure):
    _fields_ = [("n", C.c_int), ("points0", C.POINTER(C.c_double)), ("points1", C.POINTER(C.c_double)),
                ("threshold", C.c_double), ("confidence", C.c_double)]


class FmResult(C.Structure):
    _fields_ = [("inlier", C.POINTER(C.c_uint8)), ("n_inliers", C.c_int), ("hypotheses", C.c_int),
                ("F", C.c_double * 9)]


class FmFrame(C.Structure):
    _fields_ = [("d_features0", C.c_void_p), ("d_n0", C.c_void_p), ("d_features1", C.c_void_p), ("d_n1", C.c_void_p),
                ("d_idx0", C.c_void_p), ("d_idx1", C.c_void_p), ("d_idx0_out", C.c_void_p), ("d_idx1_out", C.c_void_p),
                ("threshold", C.c_double), ("confidence", C.c_double)]


class TrackConfig(C.Structure):
    _fields_ = [("max_batch", C.c_int), ("max_keypoints", C.c_int), ("device", C.c_int)]


class TrackFrameDesc(C.Structure):
    _fields_ = [("slot", C.c_int), ("d_features", C.c_void_p), ("d_n1", C.c_void_p), ("d_idx0", C.c_void_p),
                ("d_idx1", C.c_void_p), ("d_u_right", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("last_Twc", C.c_double * 16), ("th_mono_point", C.c_double), ("th_stereo_point", C.c_double),
                ("min_num_match", C.c_int)]


class TrackResult(C.Structure):
    _fields_ = [("pose_q", C.c_double * 4), ("pose_p", C.c_double * 3), ("pose_set", C.c_int),
                ("n_inliers", C.c_int), ("n_pnp_inliers", C.c_int), ("pnp_used", C.c_int), ("n_keypoints", C.c_int),
                ("n_matches", C.c_int), ("n_kept", C.c_int), ("n_mono", C.c_int), ("n_stereo", C.c_int),
                ("rounds", C.c_int), ("iterations", C.c_int * 4), ("chi2", C.c_double * 4),
                ("match_kf", C.c_void_p), ("track_id", C.c_void_p), ("kept", C.c_void_p)]


class TrackDebug(C.Structure):
    _fields_ = [("n_corr", C.c_int), ("n_mono", C.c_int), ("n_stereo", C.c_int),
                ("corr_kp", C.c_void_p), ("edge_kp", C.c_void_p), ("pnp_points", C.c_void_p),
                ("pnp_keypoints", C.c_void_p), ("edges", C.c_void_p), ("n_subsets", C.c_int),
                ("subsets", C.c_void_p), ("pnp_Rwc", C.c_double * 9), ("pnp_twc", C.c_double * 3),
                ("pnp_n_inliers", C.c_int), ("pnp_hypotheses", C.c_int), ("pnp_inlier", C.c_void_p),
                ("seed_q", C.c_double * 4), ("seed_p", C.c_double * 3), ("pnp_used", C.c_int),
                ("edge_inlier", C.c_void_p)]


class TrackLinesConfig(C.Structure):
    _fields_ = [("max_lines", C.c_int), ("max_pairs", C.c_int)]


class TrackFrameExt(C.Structure):
    _fields_ = [("d_lines", C.c_void_p), ("n_lines", C.c_int), ("kf_Twc", C.c_double * 16),
                ("kf_frame_id", C.c_int), ("frame_id", C.c_int), ("max_num_match", C.c_int),
                ("max_angle", C.c_double), ("max_distance", C.c_double), ("max_num_passed_frame", C.c_int)]


class TrackExtResult(C.Structure):
    _fields_ = [("n_lines", C.c_int), ("n_line_matches", C.c_int), ("n_line_tracks", C.c_int), ("overflow", C.c_int),
                ("tracked_well", C.c_int), ("add_keyframe", C.c_int), ("delta_angle", C.c_double),
                ("delta_distance", C.c_double), ("passed_frames", C.c_int), ("line_match_kf", C.c_void_p),
                ("line_track_id", C.c_void_p), ("line_slot", C.c_void_p)]


class TrackDebugLines(C.Structure):
    _fields_ = [("n_lines", C.c_int), ("kf_n_lines", C.c_int), ("offsets", C.c_void_p), ("point_idx", C.c_void_p),
                ("dist", C.c_void_p), ("kf_offsets", C.c_void_p), ("kf_point_idx", C.c_void_p),
                ("kf_dist", C.c_void_p)]


class KfConfig(C.Structure):
    _fields_ = [("max_batch", C.c_int), ("max_keypoints", C.c_int), ("max_tri_points", C.c_int),
                ("max_tri_observations", C.c_int), ("device", C.c_int)]


class KfFrameDesc(C.Structure):
    _fields_ = [("d_features_left", C.c_void_p), ("d_features_right", C.c_void_p), ("d_n_left", C.c_void_p),
                ("d_n_right", C.c_void_p), ("d_idx0", C.c_void_p), ("d_idx1", C.c_void_p), ("n", C.c_int),
                ("track_id", C.c_void_p), ("point_slot", C.c_void_p), ("points", C.c_void_p), ("state", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("min_x_diff", C.c_double), ("max_x_diff", C.c_double), ("max_y_diff", C.c_double),
                ("Twc", C.c_double * 16), ("next_track_id", C.c_int), ("init", C.c_int),
                ("d_table_points", C.c_void_p), ("d_table_state", C.c_void_p), ("d_table_track_id", C.c_void_p),
                ("table_capacity", C.c_int)]


class KfResult(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("n_matches", C.c_int), ("n_stereo_matches", C.c_int),
                ("n_new_ids", C.c_int), ("n_new_points", C.c_int), ("n_new_good", C.c_int),
                ("next_track_id", C.c_int), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("track_id", C.c_void_p),
                ("new_point", C.c_void_p), ("new_position", C.c_void_p)]


class RectCamera(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 12)]


class RectConfig(C.Structure):
    _fields_ = [("height", C.c_int), ("width", C.c_int), ("distortion_type", C.c_int), ("cam", RectCamera * 2),
                ("max_batch", C.c_int), ("device", C.c_int)]


class RcfConfig(C.Structure):
    _fields_ = [("max_height", C.c_int), ("max_width", C.c_int), ("max_batch", C.c_int), ("precision", C.c_int),
                ("output", C.c_int), ("device", C.c_int)]


class LmapConfig(C.Structure):
    _fields_ = [("max_bank_points", C.c_int), ("max_local_points", C.c_int), ("max_keypoints", C.c_int),
                ("max_batch", C.c_int), ("device", C.c_int), ("radius", C.c_double), ("max_distance", C.c_double),
                ("max_ratio", C.c_double)]


class LmapFrame(C.Structure):
    _fields_ = [("d_features", C.c_void_p), ("d_n1", C.c_void_p), ("d_u_right", C.c_void_p),
                ("d_point_id", C.c_void_p), ("d_point_xyz", C.c_void_p), ("d_point_good", C.c_void_p),
                ("Twc", C.c_double * 16), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("bf", C.c_double), ("width", C.c_int), ("height", C.c_int)]


class LmapResult(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("n_selected", C.c_int), ("n_projected", C.c_int),
                ("n_with_candidates", C.c_int), ("n_good", C.c_int), ("good_kp", C.c_void_p),
                ("good_point", C.c_void_p), ("assoc_id", C.c_void_p)]


class LmapHostProblem(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("features", C.c_void_p), ("u_right", C.c_void_p), ("point_id", C.c_void_p),
                ("n_local", C.c_int), ("local_ids", C.c_void_p), ("local_pos", C.c_void_p), ("local_desc", C.c_void_p),
                ("Twc", C.c_double * 16), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("bf", C.c_double), ("width", C.c_int), ("height", C.c_int),
                ("radius", C.c_double), ("max_distance", C.c_double), ("max_ratio", C.c_double)]


class LmapGlobalParams(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("max_ratio", C.c_double), ("mutual", C.c_int)]


class LmapGlobalResult(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("n_local", C.c_int), ("n_pass", C.c_int), ("n_matched", C.c_int),
                ("arg", C.c_void_p), ("best", C.c_void_p), ("second", C.c_void_p), ("match", C.c_void_p),
                ("kbest", C.c_void_p), ("match_kp", C.c_void_p), ("match_local", C.c_void_p),
                ("match_id", C.c_void_p), ("match_pos", C.c_void_p), ("match_xy", C.c_void_p)]


class LmapGlobalHostProblem(C.Structure):
    _fields_ = [("n_keypoints", C.c_int), ("features", C.c_void_p), ("n_local", C.c_int), ("local_ids", C.c_void_p),
                ("local_pos", C.c_void_p), ("local_desc", C.c_void_p)]


class PgoConfig(C.Structure):
    _fields_ = [("max_poses", C.c_int), ("max_edges", C.c_int), ("max_tiles", C.c_int), ("device", C.c_int)]


class PgoProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int), ("pose_q", C.c_void_p), ("pose_p", C.c_void_p), ("pose_fixed", C.c_void_p),
                ("n_edges", C.c_int), ("edge_i", C.c_void_p), ("edge_j", C.c_void_p), ("edge_q", C.c_void_p),
                ("edge_p", C.c_void_p), ("edge_w", C.c_void_p)]


class PgoParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("step_tol", C.c_double)]


class PgoResult(C.Structure):
    _fields_ = [("pose_q", C.c_void_p), ("pose_p", C.c_void_p), ("status", C.c_int), ("iterations", C.c_int),
                ("trials", C.c_int), ("n_free", C.c_int), ("n_tiles", C.c_int), ("n_filled_tiles", C.c_int),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("lambda_", C.c_double)]


class RsplError(RuntimeError):
    pass


_lib = None


def load(path: pathlib.Path = LIB_PATH):
    """Load librspl.so and declare the C ABI.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not path.exists():
        raise RsplError(f"{path} not built: run __graft_entry__.build() (no CPU fallback exists)")
    lib = C.CDLL(str(path))
    vp, ip, dp = C.c_void_p, C.c_int, C.c_double
    lib.rspl_last_error.restype = C.c_char_p
    lib.rspl_version.restype = C.c_char_p
    if lib.rspl_abi_version() != RSPL_ABI_VERSION:
        raise RsplError(f"{path}: ABI {lib.rspl_abi_version()}, these bindings follow ABI {RSPL_ABI_VERSION}: rebuild")
    lib.rspl_sp_create.argtypes = [C.POINTER(SpConfig), C.c_char_p, C.POINTER(vp)]
    lib.rspl_sp_infer.argtypes = [vp, vp, ip, ip, ip, vp, ip, C.POINTER(ip)]
    lib.rspl_sp_infer_device.argtypes = [vp, vp, ip, ip, ip, ip, C.c_size_t, vp, ip, vp, vp]
    lib.rspl_sp_debug_maps.argtypes = [vp, ip, vp, vp]
    lib.rspl_sp_debug_nms.argtypes = [vp, vp, ip, ip, vp]
    lib.rspl_sp_debug_layer.argtypes = [vp, ip, ip, ip, ip, vp, vp, vp, vp, ip, vp, vp]
    lib.rspl_sp_debug_select.argtypes = [vp, vp, vp, ip, ip, ip, vp, ip, vp, vp]
    lib.rspl_sp_destroy.argtypes = [vp]
    lib.rspl_sp_destroy.restype = None
    lib.rspl_device_count.argtypes = [C.POINTER(ip)]
    lib.rspl_set_device.argtypes = [ip]
    lib.rspl_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
    lib.rspl_free.argtypes = [vp]
    lib.rspl_memcpy_h2d.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rspl_memcpy_d2h.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rspl_memset.argtypes = [vp, ip, C.c_size_t, vp]
    lib.rspl_memcpy_d2d.argtypes = [vp, vp, C.c_size_t, vp]
    lib.rspl_sp_profile.argtypes = [vp, ip]
    lib.rspl_sp_stage_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ip)]
    lib.rspl_stream_create.argtypes = [C.POINTER(vp)]
    lib.rspl_stream_create_priority.argtypes = [C.POINTER(vp), ip]
    lib.rspl_stream_create_reserving.argtypes = [C.POINTER(vp), ip]
    lib.rspl_stream_destroy.argtypes = [vp]
    lib.rspl_stream_synchronize.argtypes = [vp]
    lib.rspl_event_create.argtypes = [C.POINTER(vp)]
    lib.rspl_event_record.argtypes = [vp, vp]
    lib.rspl_stream_wait_event.argtypes = [vp, vp]
    lib.rspl_event_destroy.argtypes = [vp]
    lib.rspl_timer_create.argtypes = [C.POINTER(vp)]
    lib.rspl_timer_record.argtypes = [vp, ip, vp]
    lib.rspl_timer_elapsed_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.rspl_timer_destroy.argtypes = [vp]
    lib.rspl_timer_destroy.restype = None
    if hasattr(lib, "rspl_sg_create"):
        lib.rspl_sg_create.argtypes = [C.POINTER(SgConfig), C.c_char_p, C.POINTER(vp)]
        lib.rspl_sg_infer.argtypes = [vp, vp, ip, vp, ip, vp, vp, vp, vp]
        lib.rspl_sg_infer_device.argtypes = [vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, vp]
        lib.rspl_sg_infer_device2.argtypes = [vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, vp, vp]
        lib.rspl_sg_debug_scores.argtypes = [vp, ip, vp]
        lib.rspl_sg_status.argtypes = [vp, C.POINTER(C.c_uint32)]
        lib.rspl_sg_debug_inject.argtypes = [vp, ip, C.c_uint]
        lib.rspl_sg_debug_sinkhorn.argtypes = [vp, vp, ip, ip, C.c_float, ip, vp]
        lib.rspl_sg_debug_decode.argtypes = [vp, vp, ip, ip, vp, vp, vp, vp]
        lib.rspl_sg_debug_layers.argtypes = [vp, ip, vp, vp, vp, ip, ip, vp]
        lib.rspl_sg_debug_sinkhorn_plan.argtypes = [ip, ip, ip, C.POINTER(SgSinkhornPlan)]
        lib.rspl_sg_profile.argtypes = [vp, ip]
        lib.rspl_sg_stage_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ip)]
        lib.rspl_sg_destroy.argtypes = [vp]
        lib.rspl_sg_destroy.restype = None
        lib.rspl_pm_match.argtypes = [vp, vp, ip, vp, ip, C.POINTER(DMatch), ip, C.POINTER(ip), ip]
    if hasattr(lib, "rspl_ba_create"):
        lib.rspl_ba_create.argtypes = [C.POINTER(BaConfig), C.POINTER(vp)]
        lib.rspl_ba_local.argtypes = [vp, vp, vp]
        lib.rspl_ba_submit.argtypes = [vp, vp, vp]
        lib.rspl_ba_join.argtypes = [vp, vp, vp, vp]
        lib.rspl_ba_use_reserved_cus.argtypes = [vp, ip]
        lib.rspl_ba_kernel_timing.argtypes = [vp, ip]
        lib.rspl_ba_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
        lib.rspl_ba_destroy.argtypes = [vp]
        lib.rspl_ba_destroy.restype = None
        lib.rspl_ba_debug_stage.argtypes = [vp, ip, ip, ip] + [vp] * 9
    if hasattr(lib, "rspl_ba_debug_chunk_plan"):  # (absent from older builds used as A/B baselines)
        lib.rspl_ba_debug_chunk_plan.argtypes = [ip, ip, ip, ip, C.POINTER(BaChunkPlan)]
        lib.rspl_ba_debug_chunk_geometry.argtypes = [ip, ip, ip, ip, vp, vp]
    if hasattr(lib, "rspl_ba_debug_pair_offsets"):  # (absent from older builds used as A/B baselines)
        lib.rspl_ba_debug_pair_offsets.argtypes = [vp, ip, ip, vp, ip, C.POINTER(ip)]
        lib.rspl_ba_debug_pairs.argtypes = [vp, ip, vp, ip, vp, C.c_longlong, C.POINTER(ip), C.POINTER(C.c_longlong),
                                            C.POINTER(ip)]
        lib.rspl_ba_debug_final.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "rspl_ba_trace"):  # (absent from older builds used as A/B baselines)
        lib.rspl_ba_trace.argtypes = [vp, C.POINTER(C.c_double), ip, C.POINTER(ip)]
        lib.rspl_ba_set_line_jacobian.argtypes = [vp, ip]
    if hasattr(lib, "rspl_ba_set_shard"):
        lib.rspl_ba_set_shard.argtypes = [vp, ip, ip, vp, vp]
        lib.rspl_comm_unique_id.argtypes = [vp]
        lib.rspl_comm_create.argtypes = [vp, ip, ip, ip, C.POINTER(vp)]
        lib.rspl_comm_allreduce_sum.argtypes = [vp, vp, C.c_size_t, vp]
        lib.rspl_comm_destroy.argtypes = [vp]
        lib.rspl_comm_destroy.restype = None
        lib.rspl_ba_set_comm.argtypes = [vp, vp]
        lib.rspl_group_create.argtypes = [ip, C.POINTER(vp)]
        lib.rspl_group_destroy.argtypes = [vp]
        lib.rspl_group_destroy.restype = None
        lib.rspl_ba_set_group.argtypes = [vp, vp, ip]
    if hasattr(lib, "rspl_pnp_create"):
        lib.rspl_pnp_create.argtypes = [C.POINTER(PnpConfig), C.POINTER(vp)]
        lib.rspl_pnp_solve.argtypes = [vp, vp, ip, vp]
        lib.rspl_pnp_destroy.argtypes = [vp]
        lib.rspl_pnp_destroy.restype = None
        lib.rspl_pnp_debug_hypotheses.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    if hasattr(lib, "rspl_fm_create"):
        lib.rspl_fm_create.argtypes = [C.POINTER(FmConfig), C.POINTER(vp)]
        lib.rspl_fm_destroy.argtypes = [vp]
        lib.rspl_fm_destroy.restype = None
        lib.rspl_fm_solve.argtypes = [vp, vp, ip, vp]
        lib.rspl_fm_enqueue.argtypes = [vp, ip, vp, vp]
        lib.rspl_fm_fetch.argtypes = [vp, vp]
        lib.rspl_fm_debug_subsets.argtypes = [ip, ip, vp, vp, vp, C.POINTER(C.c_int)]
        lib.rspl_fm_debug_seven_point.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
        lib.rspl_fm_debug_hypotheses.argtypes = [vp, ip, ip, vp, vp, vp]
    if hasattr(lib, "rspl_frame_create"):
        lib.rspl_frame_create.argtypes = [C.POINTER(FrameConfig), C.POINTER(vp)]
        lib.rspl_frame_optimize.argtypes = [vp, vp, ip, vp]
        lib.rspl_frame_destroy.argtypes = [vp]
        lib.rspl_frame_destroy.restype = None
    if hasattr(lib, "rspl_track_create"):
        lib.rspl_track_create.argtypes = [C.POINTER(TrackConfig), C.POINTER(vp)]
        lib.rspl_track_destroy.argtypes = [vp]
        lib.rspl_track_destroy.restype = None
        lib.rspl_track_set_keyframe.argtypes = [vp, ip, ip, vp, vp, vp, vp]
        lib.rspl_track_enqueue.argtypes = [vp, ip, vp, vp]
        lib.rspl_track_fetch.argtypes = [vp, vp]
        lib.rspl_track_debug_stage.argtypes = [vp, ip, C.POINTER(TrackDebug)]
    if hasattr(lib, "rspl_track_enable_lines"):  # (absent from older builds used as A/B baselines)
        lib.rspl_track_enable_lines.argtypes = [vp, C.POINTER(TrackLinesConfig)]
        lib.rspl_track_set_keyframe_lines.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp, vp]
        lib.rspl_track_enqueue_ext.argtypes = [vp, ip, vp, vp, vp]
        lib.rspl_track_fetch_ext.argtypes = [vp, vp, vp]
        lib.rspl_track_debug_lines.argtypes = [vp, ip, C.POINTER(TrackDebugLines)]
        lib.rspl_track_frame_lines.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, "rspl_kf_create"):
        lib.rspl_track_keyframe_table.argtypes = [vp, ip, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        lib.rspl_kf_create.argtypes = [C.POINTER(KfConfig), C.POINTER(vp)]
        lib.rspl_kf_destroy.argtypes = [vp]
        lib.rspl_kf_destroy.restype = None
        lib.rspl_kf_enqueue.argtypes = [vp, ip, vp, vp]
        lib.rspl_kf_fetch.argtypes = [vp, vp]
        lib.rspl_kf_triangulate.argtypes = [vp, ip, vp, vp, ip, vp, vp, vp, vp, vp]
    if hasattr(lib, "rspl_rect_create"):
        sz = C.c_size_t
        lib.rspl_rect_build_maps.argtypes = [C.POINTER(RectCamera), ip, ip, ip, vp, vp]
        lib.rspl_rect_debug_fixed.argtypes = [vp, vp, sz, ip, ip, vp, vp, vp]
        lib.rspl_rect_debug_sizeof.argtypes = [ip]
        lib.rspl_rect_debug_copy.argtypes = [vp, vp, sz, vp]
        lib.rspl_rect_create.argtypes = [C.POINTER(RectConfig), C.POINTER(vp)]
        lib.rspl_rect_destroy.argtypes = [vp]
        lib.rspl_rect_destroy.restype = None
        lib.rspl_rect_get_maps.argtypes = [vp, ip, vp, vp]
        lib.rspl_rect_set_maps.argtypes = [vp, ip, vp, vp]
        lib.rspl_rect_enqueue_device.argtypes = [vp, ip, vp, sz, sz, C.POINTER(ip), vp, sz, sz, vp]
        lib.rspl_rect_pair.argtypes = [vp, vp, vp, sz, vp, vp, sz]
    if hasattr(lib, "rspl_rcf_create"):
        sz = C.c_size_t
        lib.rspl_rcf_debug_sizeof.argtypes = [ip]
        lib.rspl_rcf_create.argtypes = [C.POINTER(RcfConfig), C.c_char_p, C.POINTER(vp)]
        lib.rspl_rcf_destroy.argtypes = [vp]
        lib.rspl_rcf_destroy.restype = None
        lib.rspl_rcf_infer.argtypes = [vp, vp, ip, ip, sz, vp]
        lib.rspl_rcf_infer_device.argtypes = [vp, vp, ip, ip, ip, sz, sz, vp, sz, sz, vp]
        lib.rspl_rcf_debug_logits.argtypes = [vp, ip, ip, vp]
        lib.rspl_rcf_debug_tile_rows.argtypes = [vp, ip]
        lib.rspl_rcf_profile.argtypes = [vp, ip]
        lib.rspl_rcf_stage_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(ip)]
    if hasattr(lib, "rspl_lmap_create"):
        lib.rspl_lmap_create.argtypes = [C.POINTER(LmapConfig), C.POINTER(vp)]
        lib.rspl_lmap_destroy.argtypes = [vp]
        lib.rspl_lmap_destroy.restype = None
        lib.rspl_lmap_store.argtypes = [vp, ip, vp, vp, vp, vp]
        lib.rspl_lmap_store_host.argtypes = [vp, ip, vp, vp]
        lib.rspl_lmap_bank_size.argtypes = [vp, C.POINTER(ip)]
        lib.rspl_lmap_set_local.argtypes = [vp, ip, vp, vp, vp]
        lib.rspl_lmap_enqueue.argtypes = [vp, ip, vp, vp]
        lib.rspl_lmap_fetch.argtypes = [vp, vp]
        lib.rspl_lmap_debug_points.argtypes = [vp, ip, vp, vp, vp, vp]
        lib.rspl_lmap_track_enqueue.argtypes = [vp, vp, ip, vp, vp, vp]
        lib.rspl_lmap_debug_search_host.argtypes = [C.POINTER(LmapHostProblem), vp, vp, vp, vp]
        lib.rspl_map_reference_keyframe.argtypes = [vp, ip, ip, vp, ip, C.POINTER(ip), C.POINTER(ip)]
        lib.rspl_map_local_mappoints.argtypes = [vp, ip, vp, vp, ip, C.POINTER(ip)]
    if hasattr(lib, "rspl_lmap_global_enqueue"):
        lib.rspl_lmap_global_enqueue.argtypes = [vp, ip, vp, C.POINTER(LmapGlobalParams), vp]
        lib.rspl_lmap_global_fetch.argtypes = [vp, vp]
        lib.rspl_lmap_debug_global_host.argtypes = [C.POINTER(LmapGlobalHostProblem), C.POINTER(LmapGlobalParams),
                                                    C.POINTER(LmapGlobalResult)]
        lib.rspl_lmap_debug_global_plan.argtypes = [ip, ip, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
        lib.rspl_map_good_mappoints.argtypes = [vp, vp, vp, ip, C.POINTER(ip)]
    if hasattr(lib, "rspl_pgo_create"):
        lib.rspl_pgo_create.argtypes = [C.POINTER(PgoConfig), C.POINTER(vp)]
        lib.rspl_pgo_destroy.argtypes = [vp]
        lib.rspl_pgo_destroy.restype = None
        lib.rspl_pgo_solve.argtypes = [vp, C.POINTER(PgoProblem), C.POINTER(PgoParams), C.POINTER(PgoResult)]
        lib.rspl_pgo_debug_host.argtypes = [C.POINTER(PgoProblem), C.POINTER(PgoParams), C.POINTER(PgoResult)]
        lib.rspl_pgo_debug_plan.argtypes = [C.POINTER(PgoProblem), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip),
                                            C.POINTER(ip), vp, ip]
        lib.rspl_pgo_debug_system.argtypes = [vp, C.POINTER(PgoProblem), dp, vp, vp, vp, vp]
        lib.rspl_map_pose_graph.argtypes = [vp, ip, vp, vp, vp, ip, C.POINTER(ip), vp, vp, vp, vp, vp, ip,
                                            C.POINTER(ip)]
        lib.rspl_map_apply_pose_graph.argtypes = [vp, ip, vp, vp, vp]
        lib.rspl_map_loop_candidates.argtypes = [vp, ip, ip, vp, ip, vp, vp, ip, C.POINTER(ip)]
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != RSPL_OK:
        msg = load().rspl_last_error().decode(errors="replace")
        raise RsplError(f"{what} failed (rc={rc}): {msg}")


# ---------------------------------------------------------------------------
# Device memory / stream / timer wrappers over librspl's own (system ROCm) HIP
# runtime.  Python code in this repo uses these instead of torch.cuda, so only
# one HIP runtime ever drives the device from a process.
# ---------------------------------------------------------------------------
import numpy as _np


class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self._p = C.c_void_p()
        check(load().rspl_malloc(C.byref(self._p), self.nbytes), "rspl_malloc")

    @property
    def ptr(self) -> int:
        return self._p.value

    def offset(self, nbytes: int) -> int:
        return self._p.value + int(nbytes)

    def upload(self, arr: _np.ndarray, stream=None, offset: int = 0):
        a = _np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        check(load().rspl_memcpy_h2d(self._p.value + offset, a.ctypes.data, a.nbytes, stream), "rspl_memcpy_h2d")
        return self

    def download(self, shape, dtype, stream=None, offset: int = 0) -> _np.ndarray:
        out = _np.empty(shape, dtype)
        assert offset + out.nbytes <= self.nbytes
        check(load().rspl_memcpy_d2h(out.ctypes.data, self._p.value + offset, out.nbytes, stream), "rspl_memcpy_d2h")
        return out

    def zero(self, stream=None):
        check(load().rspl_memset(self._p.value, 0, self.nbytes, stream), "rspl_memset")

    def __del__(self):
        if self._p.value:
            load().rspl_free(self._p)
            self._p = C.c_void_p()


def memcpy_d2d(dst: int, src: int, nbytes: int, stream=None):
    check(load().rspl_memcpy_d2d(dst, src, nbytes, stream), "rspl_memcpy_d2d")


def stage_times(fn_profile, fn_times, handle, nstages):
    ms = (C.c_float * nstages)()
    calls = C.c_int(0)
    check(fn_times(handle, ms, C.byref(calls)), "stage_times")
    return [ms[i] for i in range(nstages)], calls.value


class Event:
    """hipEvent (timing disabled) for cross-stream ordering."""

    def __init__(self):
        self._e = C.c_void_p()
        check(load().rspl_event_create(C.byref(self._e)), "rspl_event_create")

    def record(self, stream):
        check(load().rspl_event_record(self._e, C.c_void_p(stream)), "rspl_event_record")

    def wait_on(self, stream):
        """make `stream` wait for this event"""
        check(load().rspl_stream_wait_event(C.c_void_p(stream), self._e), "rspl_stream_wait_event")

    def __del__(self):
        if self._e.value:
            load().rspl_event_destroy(self._e)
            self._e = C.c_void_p()


class Stream:
    def __init__(self, high_priority: bool = False, reserve_cus: int = 0, priority: str = ""):
        """priority: "" (from high_priority), "high", "normal" or "low" (HIP stream priorities)."""
        self._s = C.c_void_p()
        if not priority:
            priority = "high" if high_priority else "normal"
        if reserve_cus > 0:  # CU-masked: leaves reserve_cus CUs to other (latency-bound) streams
            check(load().rspl_stream_create_reserving(C.byref(self._s), reserve_cus), "rspl_stream_create_reserving")
        elif priority in ("high", "low"):
            check(load().rspl_stream_create_priority(C.byref(self._s), 1 if priority == "high" else 0),
                  "rspl_stream_create_priority")
        else:
            check(load().rspl_stream_create(C.byref(self._s)), "rspl_stream_create")

    @property
    def handle(self) -> int:
        return self._s.value

    def synchronize(self):
        check(load().rspl_stream_synchronize(self._s), "rspl_stream_synchronize")

    def __del__(self):
        if self._s.value:
            load().rspl_stream_destroy(self._s)
            self._s = C.c_void_p()


class Timer:
    """HIP-event timer recorded on the stream the kernels run on."""

    def __init__(self):
        self._t = C.c_void_p()
        check(load().rspl_timer_create(C.byref(self._t)), "rspl_timer_create")

    def start(self, stream):
        check(load().rspl_timer_record(self._t, 0, stream.handle if isinstance(stream, Stream) else stream), "timer")

    def stop(self, stream):
        check(load().rspl_timer_record(self._t, 1, stream.handle if isinstance(stream, Stream) else stream), "timer")

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        check(load().rspl_timer_elapsed_ms(self._t, C.byref(ms)), "rspl_timer_elapsed_ms")
        return ms.value

    def __del__(self):
        if self._t.value:
            load().rspl_timer_destroy(self._t)
            self._t = C.c_void_p()


def device_count() -> int:
    n = C.c_int(0)
    rc = load().rspl_device_count(C.byref(n))
    return n.value if rc == RSPL_OK else 0


def synchronize():
    check(load().rspl_device_synchronize(), "rspl_device_synchronize")
