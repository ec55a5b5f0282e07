"""ctypes mirrors of the POD structs in include/scavislam_hip.h (the test oracle declares the same layouts independently).

Names follow the reference's domain: FastGridCell grids (keyframes.h:31-44), CandidatePoint
(data_structures.h:37-69), the BA edge records of SlamGraph::copyDataToG2o
(slam_graph.cpp:983-1032).
"""
import ctypes as C

import numpy as np

SVS_MAX_CELLS = 64


class Cam(C.Structure):
    """Per-level StereoCamera (frame_grabber-impl.cpp:48-60)."""
    _fields_ = [("f", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("b", C.c_double),
                ("w", C.c_int32), ("h", C.c_int32)]


class FastGrid(C.Structure):
    """FastGrid members (fast_grid.cpp:23-58)."""
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("cell_w", C.c_int32), ("cell_h", C.c_int32),
                ("min_inner", C.c_int32), ("min_outer", C.c_int32),
                ("max_inner", C.c_int32), ("max_outer", C.c_int32),
                ("fast_min", C.c_int32), ("fast_max", C.c_int32),
                ("thr", C.c_int32 * SVS_MAX_CELLS)]


CANDIDATE_DTYPE = np.dtype([("xyz_anchor", "<f8", 3), ("anchor_obs_pyr", "<f8", 3),
                            ("anchor_level", "<i4"), ("kf_index", "<i4"),
                            ("point_id", "<i4"), ("pad_", "<i4")], align=True)
assert CANDIDATE_DTYPE.itemsize == 64

MATCH_RESULT_DTYPE = np.dtype([("status", "<i4"), ("u", "<i4"), ("v", "<i4"), ("znssd", "<i4"),
                               ("obs", "<f8", 3), ("xyz_actkey", "<f8", 3)], align=True)
assert MATCH_RESULT_DTYPE.itemsize == 64

KEYFRAME_DTYPE = np.dtype([("T_anchor_from_w", "<f8", 12), ("pyr", "<u8", 3),
                           ("stride", "<i4", 3), ("pad_", "<i4")], align=True)
assert KEYFRAME_DTYPE.itemsize == 136

DENSE_SUMS_DTYPE = np.dtype([("H", "<f8", 21), ("b", "<f8", 6), ("chi2", "<f8"),
                             ("n_valid", "<i8")], align=True)
assert DENSE_SUMS_DTYPE.itemsize == 232

# svs_dense_lm_record: one entry per chi2 evaluation of DenseTracker::denseTrackingGpu (dense_tracking.cpp:60-193)
DENSE_LM_RECORD_DTYPE = np.dtype([("level", "<i4"), ("accepted", "<i4"), ("chi2", "<f4"), ("new_chi2", "<f4")])
assert DENSE_LM_RECORD_DTYPE.itemsize == 16

BA_EDGE_DTYPE = np.dtype([("obs", "<f8", 3), ("info", "<f8", 3), ("point", "<i4"),
                          ("pose", "<i4"), ("anchor", "<i4"), ("pad_", "<i4")], align=True)
assert BA_EDGE_DTYPE.itemsize == 64

BA_CONSTRAINT_DTYPE = np.dtype([("T_21", "<f8", 12), ("info", "<f8", 36),
                                ("pose1", "<i4"), ("pose2", "<i4")], align=True)
assert BA_CONSTRAINT_DTYPE.itemsize == 392


class BaParams(C.Structure):
    """OptParams (slam_graph.hpp:36-50) + the g2o settings of setupG2o/optimize."""
    _fields_ = [("num_iters", C.c_int32), ("use_robust", C.c_int32), ("huber_delta", C.c_double),
                ("lambda_init", C.c_double), ("max_trials", C.c_int32),
                ("self_edge_mode", C.c_int32)]

    @classmethod
    def reference_defaults(cls):
        # backend.cpp:187 OptParams(2,true,3); delta stays 1 (slam_graph-impl.cpp:86-90);
        # lambda 50 (slam_graph.cpp:338); maxTrialsAfterFailure 5 (slam_graph.cpp:1073)
        return cls(2, 1, 1.0, 50.0, 5, 0)


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("accepted", C.c_int32),
                ("terminated", C.c_int32), ("chi2_init", C.c_double), ("chi2_final", C.c_double),
                ("lambda_final", C.c_double)]


MATCH_OK, MATCH_NO_ANCHOR, MATCH_BORDER, MATCH_DEPTH, MATCH_TEXTURE, MATCH_NONE, MATCH_NO_DISP, MATCH_SKIPPED = range(8)


def level_cams(f, cx, cy, b, w, h, levels=3):
    """cam_vec of FrameGrabber<StereoCamera> (frame_grabber-impl.cpp:48-60)."""
    out = (Cam * levels)()
    for l in range(levels):
        s = float(1 << l)
        out[l] = Cam(f / s, cx / s, cy / s, b * (1 << l), int(w / s), int(h / s))
    return out


class StereoParams(C.Structure):
    """svs_stereo_params: cv::StereoBM state as set at stereo_frontend.cpp:620-653."""
    _fields_ = [("prefilter_cap", C.c_int32), ("sad_window", C.c_int32), ("min_disparity", C.c_int32),
                ("num_disparities", C.c_int32), ("texture_threshold", C.c_int32), ("uniqueness_ratio", C.c_int32),
                ("speckle_window", C.c_int32), ("speckle_range", C.c_int32), ("disp12_max_diff", C.c_int32)]

    @classmethod
    def reference(cls, num_disp16=2):
        return cls(31, 7, 0, 16 * num_disp16, 10, 15, 100, 32, 1)


class PoseOptParams(C.Structure):
    """svs_pose_opt_params: PoseOptimizerParams (pose_optimizer.h:36-58)."""
    _fields_ = [("robust_kernel", C.c_int32), ("num_iter", C.c_int32), ("kernel_param", C.c_double),
                ("initial_mu", C.c_double), ("tau", C.c_double), ("min_obs", C.c_int32), ("pad_", C.c_int32)]

    @classmethod
    def reference(cls):
        """PoseOptimizerParams(true, 2, 15) as passed at stereo_frontend.cpp:1061"""
        return cls(1, 15, 2.0, -1.0, 1e-5)


class PoseOptStats(C.Structure):
    _fields_ = [("initial_chi2", C.c_double), ("chi2", C.c_double), ("max_err", C.c_double),
                ("num_obs", C.c_int32), ("status", C.c_int32)]


# svs_gated_point / svs_point_stats: StereoFrontend::processMatchedPoints (stereo_frontend.cpp:834-974)
GATED_POINT_DTYPE = np.dtype([("accepted", "<i4"), ("is_new", "<i4"), ("uv_pyr", "<f8", 2), ("curkey_uv_pyr", "<f8", 2)])
assert GATED_POINT_DTYPE.itemsize == 40
POINT_STATS_DTYPE = np.dtype([("num_points_grid2x2", "<i4", 4), ("num_points_grid3x3", "<i4", 9), ("num_matched_points", "<i4", 3),
                              ("num_track_points", "<i4"), ("num_obs", "<i4"), ("pad_", "<i4", 2), ("sum_track_length", "<f8")])
assert POINT_STATS_DTYPE.itemsize == 88


class LoopCheck(C.Structure):
    """svs_loop_check: one geometric check (PlaceRecognizer::geometricCheck, placerecognizer.cpp:175-202)."""
    _fields_ = [("query_slot", C.c_int32), ("train_slot", C.c_int32), ("n_hyp", C.c_int32), ("pixel_thr", C.c_double), ("seed", C.c_uint64),
                ("h_samples", C.c_void_p)]


class LoopResult(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("best_hyp", C.c_int32), ("n_invalid_hyp", C.c_int32),
                ("T_query_from_train", C.c_double * 12)]


class LoopLocation(C.Structure):
    """svs_loop_location: one place on its way into the index (PlaceRecognizer::addLocation, placerecognizer.cpp:248-318)."""
    _fields_ = [("slot", C.c_int32), ("do_loop_detection", C.c_int32), ("h_exclude", C.c_void_p), ("n_exclude", C.c_int32), ("radius", C.c_float),
                ("min_score", C.c_float)]


class LoopLocationResult(C.Structure):
    _fields_ = [("number_of_words", C.c_int32), ("n_scored", C.c_int32), ("best_slot", C.c_int32), ("best_score", C.c_float), ("candidate", C.c_int32)]


class VocabParams(C.Structure):
    """svs_vocab_params: what svs_vocab_train clusters into (create_dictionary.cpp:144-177: 11 iterations, k-means++ centres)."""
    _fields_ = [("n_words", C.c_int32), ("iterations", C.c_int32), ("seed", C.c_uint64), ("h_init", C.c_void_p), ("drop_empty", C.c_int32)]


class VocabResult(C.Structure):
    _fields_ = [("n_words_out", C.c_int32), ("n_seeded", C.c_int32), ("iterations_run", C.c_int32), ("converged", C.c_int32), ("n_empty", C.c_int32),
                ("inertia_q28", C.c_uint64)]


class SurfParams(C.Structure):
    """svs_surf_params: SurfFeatureDetector(600, 2) / SurfDescriptorExtractor(2, 4, 2, false) of placerecognizer.cpp:216, :240."""
    _fields_ = [("hessian_threshold", C.c_float), ("n_octaves", C.c_int32), ("n_octave_layers", C.c_int32), ("require_disparity", C.c_int32)]

    @classmethod
    def reference(cls, hessian_threshold=600.0, n_octaves=2, n_octave_layers=2, require_disparity=True):
        return cls(hessian_threshold, n_octaves, n_octave_layers, int(bool(require_disparity)))


# svs_surf_keypoint
SURF_KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("laplacian", "<i4"),
                                ("pad_", "<i4")])
assert SURF_KEYPOINT_DTYPE.itemsize == 32
SURF_STAGES = 6


class SeedParams(C.Structure):
    """svs_seed_params: params_.newpoint_clearance, ui.num_max_points, ui.min_num_points, USE_N_LEVELS_FOR_MATCHING (stereo_frontend.cpp:319-331, :735-749)."""
    _fields_ = [("clearance", C.c_int32), ("num_max_points", C.c_int32), ("min_num_points", C.c_int32), ("n_levels", C.c_int32)]

    @classmethod
    def reference(cls, clearance=2, num_max_points=300, min_num_points=25, n_levels=3):
        return cls(clearance, num_max_points, min_num_points, n_levels)

    def max_records(self):
        """the most one problem can produce = the smallest output capacity the library accepts"""
        return sum((self.num_max_points >> l) + 1 for l in range(self.n_levels))


# svs_seed_problem: one problem of svs_seed_points (device memory)
SEED_PROBLEM_DTYPE = np.dtype([("T_newkey_from_cur", "<f8", 12), ("seed", "<u8"), ("add_flags", "<i4", 9), ("n0", "<i4", 3), ("n_tree", "<i4"),
                               ("kf_index", "<i4"), ("first_point_id", "<i4"), ("use_order", "<i4"), ("n_order", "<i4", 3), ("pad_", "<i4")])
assert SEED_PROBLEM_DTYPE.itemsize == 184


class SeedArgs(C.Structure):
    """svs_seed_args: device pointers of a batch of seeding problems"""
    _fields_ = [("d_xy", C.c_void_p * 3), ("xy_bstride", C.c_size_t * 3), ("xy_cap", C.c_int32 * 3),
                ("d_n", C.c_void_p * 3), ("n_bstride", C.c_size_t * 3),
                ("d_cell_count", C.c_void_p * 3), ("cell_bstride", C.c_size_t * 3), ("n_cells", C.c_int32 * 3),
                ("d_disp", C.c_void_p), ("disp_stride", C.c_int32), ("disp_bstride", C.c_size_t),
                ("cam", Cam), ("d_prob", C.c_void_p),
                ("d_tree_xy", C.c_void_p), ("d_tree_level", C.c_void_p), ("tree_bstride", C.c_size_t),
                ("d_order", C.c_void_p * 3), ("order_bstride", C.c_size_t * 3), ("batch", C.c_int32)]


SEED_FIRST, SEED_MORE = 0, 1


class SeedRequest(C.Structure):
    """svs_seed_request: one new keyframe of one stream for svs_frontend_seed_keyframes"""
    _fields_ = [("stream", C.c_int32), ("mode", C.c_int32), ("kf_index", C.c_int32), ("first_point_id", C.c_int32),
                ("T_newkey_from_cur", C.c_double * 12), ("seed", C.c_uint64), ("h_order", C.c_void_p * 3), ("n_order", C.c_int32 * 3), ("pad_", C.c_int32)]


# ---- back end: re-registration of a keyframe (svs_reg_*; Backend::localRegisterFrame / globalLoopClosure, backend.cpp:549-611, 830-1001)
REG_LOCAL, REG_LOOP = 0, 1
REG_OK, REG_FEW_CANDIDATES, REG_FEW_MATCHES_PASS1, REG_FEW_MATCHES_PASS2, REG_NOT_COVISIBLE = range(5)
REG_KF_IN_WINDOW, REG_KF_DIRECT_NEIGHBOR = 1, 2
REG_STAGES = 7


class RegParams(C.Structure):
    """svs_reg_params: covis_thr, the two search radii / iteration counts of matchAndAlign (backend.cpp:735-779), REPROJ_THR (:625)."""
    _fields_ = [("covis_thr", C.c_int32), ("search_radius", C.c_int32 * 2), ("thr_mean", C.c_int32), ("thr_std", C.c_int32), ("num_iter", C.c_int32 * 2),
                ("pad_", C.c_int32), ("reproj_thr", C.c_double), ("kernel_param", C.c_double)]

    @classmethod
    def reference(cls, covis_thr=15):
        return cls(covis_thr, (C.c_int32 * 2)(10, 4), 22, 10, (C.c_int32 * 2)(25, 15), 0, 2.0, 2.0)


class RegRequest(C.Structure):
    """svs_reg_request: one root keyframe with its keyframe table, source points and (local mode) observer table"""
    _fields_ = [("mode", C.c_int32), ("n_kf", C.c_int32), ("n_src", C.c_int32), ("root_kf", C.c_int32),
                ("d_root_disp", C.c_void_p), ("root_disp_stride", C.c_int32), ("pad_", C.c_int32),
                ("fast_thr", (C.c_int32 * SVS_MAX_CELLS) * 3), ("T_root_from_world", C.c_double * 12),
                ("h_kfs", C.c_void_p), ("h_kf_flags", C.c_void_p), ("h_src", C.c_void_p), ("h_obs_begin", C.c_void_p), ("h_obs_kf", C.c_void_p)]


class RegResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_candidates", C.c_int32), ("n_obs_pass1", C.c_int32), ("n_obs_pass2", C.c_int32), ("n_accepted", C.c_int32),
                ("n_qualified", C.c_int32), ("T_newroot_from_oldroot", C.c_double * 12), ("T_pass1", C.c_double * 12),
                ("stats_pass1", PoseOptStats), ("stats_pass2", PoseOptStats)]


REG_KF_STATS_DTYPE = np.dtype([("strength", "<i4"), ("n_u_hi", "<i4"), ("n_u_lo", "<i4"), ("n_v_hi", "<i4"), ("n_v_lo", "<i4"), ("qualifies", "<i4"),
                               ("in_vertex_table", "<i4"), ("pad_", "<i4")])
assert REG_KF_STATS_DTYPE.itemsize == 32


# ---- back end: the device-resident map and requests by ids (svs_map_*, svs_reg_register_map_batch)
REG_OVER_CAPACITY = 5
MAP_MAX_KEYFRAMES = 16384


class RegMapRequest(C.Structure):
    """svs_reg_map_request: a root keyframe by id, with the ids of framesInNeighborhood(root) and directNeighborsOf(root)"""
    _fields_ = [("mode", C.c_int32), ("root_kf", C.c_int32), ("n_walk", C.c_int32), ("n_direct", C.c_int32), ("T_root_from_world", C.c_double * 12),
                ("h_walk_kf", C.c_void_p), ("h_direct_kf", C.c_void_p)]


# ---- front end: a stream's neighbourhood list from the map (svs_frontend_set_candidates_from_map)
class NbhRequest(C.Structure):
    """svs_nbh_request: the stream, the vertex list (ids, root first), the stream's slot table (id per slot, -1 for none) and the new-point groups from the host"""
    _fields_ = [("stream", C.c_int32), ("n_vertex", C.c_int32), ("n_head", C.c_int32), ("n_head_groups", C.c_int32), ("h_vertex_kf", C.c_void_p),
                ("h_slot_kf", C.c_void_p), ("h_head_group_end", C.c_void_p), ("h_head", C.c_void_p)]


class NbhResult(C.Structure):
    """svs_nbh_result"""
    _fields_ = [("n_points", C.c_int32), ("n_map_points", C.c_int32), ("n_vertex", C.c_int32), ("n_no_slot", C.c_int32), ("over_capacity", C.c_int32),
                ("pad_", C.c_int32 * 3)]


assert C.sizeof(NbhRequest) == 48 and C.sizeof(NbhResult) == 32


# ---- front end: a stream's whole neighbourhood from a root id (svs_frontend_set_neighborhood_from_root)
class NbrRequest(C.Structure):
    """svs_nbr_request: the stream, the root and the active keyframe by id, findNeighborsOfRoot's cap, the stream's slot table, the head's groups (the first
    n_fixed_groups stay, every later one is keyed by a keyframe id)"""
    _fields_ = [("stream", C.c_int32), ("root_id", C.c_int32), ("act_id", C.c_int32), ("max_num_neighbors", C.c_int32), ("n_head", C.c_int32),
                ("n_head_groups", C.c_int32), ("n_fixed_groups", C.c_int32), ("pad_", C.c_int32), ("h_slot_kf", C.c_void_p), ("h_head_group_end", C.c_void_p),
                ("h_head", C.c_void_p), ("h_head_group_kf", C.c_void_p)]


class NbrResult(C.Structure):
    """svs_nbr_result"""
    _fields_ = [("n_points", C.c_int32), ("n_map_points", C.c_int32), ("n_vertex", C.c_int32), ("n_no_slot", C.c_int32), ("over_capacity", C.c_int32),
                ("root_outside_window", C.c_int32), ("n_root_neighbors", C.c_int32), ("n_no_path", C.c_int32), ("act_index", C.c_int32),
                ("n_act_neighbors", C.c_int32), ("n_head_kept", C.c_int32), ("n_head_dropped", C.c_int32), ("n_groups", C.c_int32), ("pad_", C.c_int32 * 3)]


NBR_RESULT_FIELDS = tuple(f for f, _ in NbrResult._fields_ if f != "pad_")
assert C.sizeof(NbrRequest) == 64 and C.sizeof(NbrResult) == 64


# ---- back end: the double window's BA problem from the map (svs_map_prepare_window)
class MapWindowResult(C.Structure):
    """svs_map_window_result: final window, W0, active points (-1: the final window exceeded window_cap), upper bound of the window's edges"""
    _fields_ = [("n_window", C.c_int32), ("n_initial", C.c_int32), ("n_active", C.c_int32), ("n_edges_bound", C.c_int32)]


assert C.sizeof(MapWindowResult) == 16
MAP_WINDOW_MAX = 256      # the solve's limit on a window's keyframes


# ---- back end: the pose graph's edges in the map and their constraints (svs_map_add_edges .. svs_map_compute_constraints)
MAP_EDGE_DTYPE = np.dtype([("lo", "<i4"), ("hi", "<i4"), ("strength", "<i4"), ("edge_type", "<i4"), ("is_marginalized", "<i4"), ("pad_", "<i4"),
                           ("T_lo_from_hi", "<f8", 12), ("info", "<f8", 36)])
MAP_CONSTRAINT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("strength", "<i4"), ("n_missing", "<i4"), ("pad_", "<i4"), ("median", "<f8"), ("norm_dist", "<f8"),
                                        ("T_12", "<f8", 12), ("info", "<f8", 36)])
assert MAP_EDGE_DTYPE.itemsize == 408 and MAP_CONSTRAINT_RESULT_DTYPE.itemsize == 416
EDGE_LOCAL, EDGE_METRIC, EDGE_APPEARANCE = 0, 1, 2
CONS_OK, CONS_EMPTY, CONS_MISSING_ANCHOR = 0, 1, 2
WALK_OK, WALK_NO_PATH = 0, 1          # svs_map_absolute_poses
MAP_WALK_MAX_REQUESTS = 256           # requests of one walk call
MAP_CONS_MAX_REQUESTS = 256


class MapConstraintRequest(C.Structure):
    """svs_map_constraint_request: computeConstraint(kf1, kf2), up to two pose overrides, the caller's cached anchor poses (ids strictly ascending)"""
    _fields_ = [("kf1", C.c_int32), ("kf2", C.c_int32), ("store", C.c_int32), ("n_override", C.c_int32), ("override_id", C.c_int32 * 2), ("n_cached", C.c_int32),
                ("pad_", C.c_int32), ("override_T", (C.c_double * 12) * 2), ("cached_ids", C.c_void_p), ("cached_T", C.c_void_p)]


assert C.sizeof(MapConstraintRequest) == 240


# ---- back end: inserting a keyframe into the map (svs_map_compute_strength, svs_map_add_keyframe, svs_map_get_points, svs_map_get_feature_table)
MAP_ADDKF_MAX_NEIGHBORS = 1024
MAP_NEW_POINT_DTYPE = np.dtype([("xyz_anchor", "<f8", 3), ("anchor_obs_pyr", "<f8", 3), ("feat_center", "<f8", 3), ("point_id", "<i4"), ("anchor_id", "<i4"),
                                ("anchor_level", "<i4"), ("feat_level", "<i4"), ("pad_", "<i4", 2)])
MAP_TRACK_POINT_DTYPE = np.dtype([("center", "<f8", 3), ("global_id", "<i4"), ("level", "<i4")])
MAP_KEY_DTYPE = np.dtype([("kf_id", "<i4"), ("strength", "<i4"), ("n_left", "<i4"), ("n_right", "<i4"), ("n_top", "<i4"), ("n_bottom", "<i4"), ("edge", "<i4"),
                          ("pad_", "<i4")])
assert MAP_NEW_POINT_DTYPE.itemsize == 96 and MAP_TRACK_POINT_DTYPE.itemsize == 32 and MAP_KEY_DTYPE.itemsize == 32


class MapStrengthResult(C.Structure):
    """svs_map_strength_result"""
    _fields_ = [("n_keys", C.c_int32), ("m", C.c_int32), ("over_capacity", C.c_int32), ("n_edges", C.c_int32)]


class RegCommitResult(C.Structure):
    """svs_reg_commit_result: what svs_reg_commit / svs_map_register_keyframes / svs_map_add_loop_closure did to the map"""
    _fields_ = [("committed", C.c_int32), ("mode", C.c_int32), ("root_id", C.c_int32), ("other_id", C.c_int32), ("n_track", C.c_int32),
                ("n_pairs_added", C.c_int32), ("n_edges", C.c_int32), ("status", C.c_int32), ("T_new", C.c_double * 12)]


assert C.sizeof(RegCommitResult) == 128


class KeyframeC(C.Structure):
    """svs_keyframe (KEYFRAME_DTYPE as a ctypes structure)"""
    _fields_ = [("T_anchor_from_w", C.c_double * 12), ("pyr", C.c_void_p * 3), ("stride", C.c_int32 * 3), ("pad_", C.c_int32)]


class MapAddKeyframeArgs(C.Structure):
    """svs_map_add_keyframe_args"""
    _fields_ = [("newkey_id", C.c_int32), ("oldkey_id", C.c_int32), ("covis_thr", C.c_int32), ("half_width", C.c_int32), ("half_height", C.c_int32),
                ("disp_stride", C.c_int32), ("n_new", C.c_int32), ("n_track", C.c_int32), ("T_newkey_from_oldkey", C.c_double * 12), ("keyframe", KeyframeC),
                ("disp", C.c_void_p), ("fast_thr", C.c_void_p), ("new_points", C.c_void_p), ("track_points", C.c_void_p), ("cached_ids", C.c_void_p),
                ("cached_T", C.c_void_p), ("n_cached", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(KeyframeC) == 136 and C.sizeof(MapAddKeyframeArgs) == 32 + 96 + 136 + 48 + 8


class CommitKeyframeRequest(C.Structure):
    """svs_commit_keyframe_request: one stream's SVS_KF_DROP decision applied to the map (svs_frontend_commit_keyframe)"""
    _fields_ = [("stream", C.c_int32), ("slot", C.c_int32), ("newkey_id", C.c_int32), ("oldkey_id", C.c_int32), ("covis_thr", C.c_int32), ("half_width", C.c_int32),
                ("half_height", C.c_int32), ("disp_stride", C.c_int32), ("disp", C.c_void_p), ("h_fast_thr", C.c_void_p), ("cached_ids", C.c_void_p),
                ("cached_T", C.c_void_p), ("n_cached", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(CommitKeyframeRequest) == 72


# ---- front end: the keyframe switch / drop decision behind a step (svs_keyframe_decide, svs_frontend_set_vertex_table, svs_frontend_decide_keyframes)
KF_MAX_VERTICES, KF_MAX_STRENGTH, KF_MAX_SLOTS, KF_SET_MAP = 64, 64, 1024, -1
KF_KEEP, KF_SWITCH, KF_DROP = 0, 1, 2
KF_VERTEX_DTYPE = np.dtype([("T_me_from_w", "<f8", 12), ("kf_id", "<i4"), ("set_begin", "<i4"), ("set_count", "<i4"), ("pad_", "<i4")])
KF_TABLE_DTYPE = np.dtype([("n_vertex", "<i4"), ("act", "<i4"), ("n_neighbors", "<i4"), ("pad_", "<i4"), ("neighbors", "<i4", KF_MAX_VERTICES)])
KEYFRAME_DECISION_DTYPE = np.dtype([("valid", "<i4"), ("decision", "<i4"), ("n_new", "<i4"), ("n_track", "<i4"), ("closest_index", "<i4"), ("closest_id", "<i4"),
                                    ("shared", "<i4"), ("featureless", "<i4"), ("closest_dist", "<f8"), ("av_track_length", "<f8"), ("T_cur_after", "<f8", 12),
                                    ("T_newkey_from_w", "<f8", 12), ("add_flags", "<i4", 9), ("n_strength", "<i4"), ("over_capacity", "<i4"), ("pad_", "<i4"),
                                    ("strength_kf", "<i4", KF_MAX_STRENGTH), ("strength_count", "<i4", KF_MAX_STRENGTH)])
assert KF_VERTEX_DTYPE.itemsize == 112 and KF_TABLE_DTYPE.itemsize == 272 and KEYFRAME_DECISION_DTYPE.itemsize == 800


class KeyframeDecideParams(C.Structure):
    """svs_keyframe_decide_params: ui.parallax_thr (a float), the count of shallWeSwitchKeyframe (:503), the cell minimum and corner count of
    shallWeDropNewKeyframe (:519, :525), its track-length bound (:527), params_.covis_thr, ui.min_num_points"""
    _fields_ = [("parallax_thr", C.c_float), ("switch_min_shared", C.c_int32), ("featureless_cell_min", C.c_int32), ("featureless_corners_thr", C.c_int32),
                ("max_av_track_length", C.c_double), ("covis_thr", C.c_int32), ("min_num_points", C.c_int32)]

    @classmethod
    def reference(cls):
        return cls(0.75, 100, 15, 2, 75.0, 15, 25)


class KeyframeDecideArgs(C.Structure):
    """svs_keyframe_decide_args: device pointers of a batch of streams"""
    _fields_ = [("d_res", C.c_void_p), ("res_bstride", C.c_size_t), ("d_pts", C.c_void_p), ("pts_bstride", C.c_size_t), ("d_gated", C.c_void_p),
                ("gated_bstride", C.c_size_t), ("d_stats", C.c_void_p), ("d_T_cur_from_actkey", C.c_void_p), ("d_tracking_ok", C.c_void_p), ("d_n", C.c_void_p),
                ("n", C.c_int32), ("batch", C.c_int32), ("d_table", C.c_void_p), ("d_vertex", C.c_void_p), ("vertex_bstride", C.c_size_t),
                ("d_set_ids", C.c_void_p), ("set_bstride", C.c_size_t), ("d_slot_kf", C.c_void_p), ("slot_bstride", C.c_size_t), ("max_keyframes", C.c_int32),
                ("pad_", C.c_int32), ("map", C.c_void_p)]


class VertexRequest(C.Structure):
    """svs_vertex_request: one stream's vertex table for svs_frontend_set_vertex_table (host pointers)"""
    _fields_ = [("stream", C.c_int32), ("n_vertex", C.c_int32), ("act", C.c_int32), ("n_neighbors", C.c_int32), ("h_vertex_kf", C.c_void_p),
                ("h_vertex_T", C.c_void_p), ("h_set_begin", C.c_void_p), ("h_set_count", C.c_void_p), ("h_set_ids", C.c_void_p), ("h_neighbors", C.c_void_p),
                ("h_slot_kf", C.c_void_p), ("n_set_ids", C.c_int32), ("pad_", C.c_int32)]


assert C.sizeof(KeyframeDecideParams) == 32 and C.sizeof(KeyframeDecideArgs) == 160 and C.sizeof(VertexRequest) == 80


# ---- front end: newpoint_map on the device (svs_frontend_newpoints_*, svs_newpoints_prune, svs_frontend_seed_newpoints, svs_frontend_set_candidates_from_newpoints)
NEWPOINTS_MAX_GROUPS = 64
NEWPOINTS_PREPEND, NEWPOINTS_REPLACE = 0, 1


class NewpointsPutRequest(C.Structure):
    """svs_newpoints_put_request: a group's records from the host"""
    _fields_ = [("stream", C.c_int32), ("kf_id", C.c_int32), ("mode", C.c_int32), ("n", C.c_int32), ("h_records", C.c_void_p)]


class NewpointsPruneArgs(C.Structure):
    """svs_newpoints_prune_args: device pointers of a batch of streams"""
    _fields_ = [("d_res", C.c_void_p), ("res_bstride", C.c_size_t), ("d_pts", C.c_void_p), ("pts_bstride", C.c_size_t), ("d_gated", C.c_void_p),
                ("gated_bstride", C.c_size_t), ("d_n", C.c_void_p), ("d_n_new", C.c_void_p), ("n", C.c_int32), ("batch", C.c_int32),
                ("d_store", C.c_void_p), ("store_bstride", C.c_size_t), ("d_group_count", C.c_void_p), ("group_bstride", C.c_size_t),
                ("d_n_groups", C.c_void_p), ("d_stream", C.c_void_p)]


class NewpointsDropRequest(C.Structure):
    """svs_newpoints_drop_request"""
    _fields_ = [("stream", C.c_int32), ("n_keys", C.c_int32), ("h_keys", C.c_void_p)]


class NewpointsListRequest(C.Structure):
    """svs_newpoints_list_request: the hand-over of one stream (host pointers)"""
    _fields_ = [("stream", C.c_int32), ("n_keys", C.c_int32), ("n_tail", C.c_int32), ("pad_", C.c_int32), ("h_keys", C.c_void_p), ("h_slot_kf", C.c_void_p),
                ("h_tail", C.c_void_p)]


class NewpointsListResult(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_head", C.c_int32), ("n_groups", C.c_int32), ("n_no_slot", C.c_int32), ("over_capacity", C.c_int32),
                ("pad_", C.c_int32 * 3)]


NEWPOINTS_LIST_RESULT_FIELDS = tuple(f for f, _ in NewpointsListResult._fields_ if f != "pad_")
assert C.sizeof(NewpointsPutRequest) == 24 and C.sizeof(NewpointsPruneArgs) == 120 and C.sizeof(NewpointsDropRequest) == 16
assert C.sizeof(NewpointsListRequest) == 40 and C.sizeof(NewpointsListResult) == 32


# ---- matcher: optional sub-pixel refinement of a match (svs_match_subpixel, svs_frontend_set_subpixel)
class SubpixParams(C.Structure):
    """svs_subpix_params: Gauss-Newton steps at most, the bound on |offset| per axis (in (0, 2]), the step size below which the iteration stops"""
    _fields_ = [("iterations", C.c_int32), ("max_shift", C.c_float), ("eps", C.c_float), ("pad_", C.c_int32)]

    @classmethod
    def default(cls, iterations=8, max_shift=1.5, eps=0.03):
        return cls(iterations, max_shift, eps, 0)


SUBPIX_INFO_DTYPE = np.dtype([("dx", "<f4"), ("dy", "<f4"), ("n_iter", "<i4"), ("state", "<i4")])
SUBPIX_REFINED, SUBPIX_UNTOUCHED, SUBPIX_SINGULAR, SUBPIX_SHIFT, SUBPIX_NO_DISP = range(5)
assert C.sizeof(SubpixParams) == 16 and SUBPIX_INFO_DTYPE.itemsize == 16
