"""orbx -- Python host binding of liborbx.so (the MI355X ORB front end).

Thin ctypes layer over the C ABI in include/orbx.h.  It mirrors the
reference interfaces for tests and the benchmark:

  Extractor      ORB_SLAM2::ORBextractor  (/root/reference/include/ORBextractor.h:25-91)
  search_by_bow  ORBmatcher::SearchByBoW(KF, KF) (/root/reference/src/ORBmatcher.cc:278-366)
  search_for_triangulation  ORBmatcher::SearchForTriangulation, batched (ORBmatcher.cc:368-467)
  keyframe_search  the search of ORBmatcher::Fuse / SearchBySim3, batched (ORBmatcher.cc:532-551)
  keyframe_project / KeyframePlan  their projection on the device, and both on device tensors
  search_for_initialization  ORBmatcher::SearchForInitialization, batched (ORBmatcher.cc:197-276)
  compute_stereo_matches  Frame::ComputeStereoMatches (/root/reference/src/Frame.cc:446-620)
  descriptor_distance_batch  ORBmatcher::DescriptorDistance (ORBmatcher.cc:896-908)
  Plan / MatchPlan  batched device-resident throughput path (bench.py)

The library is mandatory: importing this package raises if liborbx.so is
missing, and every compute call runs the HIP kernels (there is no CPU path).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "liborbx.so")
if os.environ.get("ORBX_VARIANT"):  # profiling only: tools/variant.sh builds liborbx_<name>.so
    LIB_PATH = os.path.join(os.path.dirname(HERE), "liborbx_%s.so" % os.environ["ORBX_VARIANT"])

if not os.path.exists(LIB_PATH):
    raise ImportError("liborbx.so not built (%s): run __graft_entry__.build() or "
                      "make -C orb-slam-system_amd" % LIB_PATH)

try:
    # Load torch (and its bundled libamdhip64.so.7) first: liborbx.so then binds to the
    # same HIP runtime by SONAME, so one process never holds two HIP runtimes.
    import torch as _torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is plumbing only
    _torch = None

_lib = ctypes.CDLL(LIB_PATH)

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28

OK, ERR_ARG, ERR_CELL_ROI, ERR_LEVEL_SIZE, ERR_QUADTREE, ERR_CAPACITY, ERR_UNSUPPORTED, \
    ERR_HIP, ERR_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6, -7, -8
ORBV_QUERY_GATED = 1  # orbv_db_query_batch flags (include/orbx.h)
ORBM_PLAN_ZERO_TAIL, ORBM_PLAN_VALU, ORBM_PLAN_NO_FOLD = 1, 2, 4  # orbm_plan_set_options flags (include/orbx.h)
ORBX_PLAN_PYR_TILES, ORBX_PLAN_BRIEF_PATCH, ORBX_PLAN_BRIEF_LEVEL, ORBX_PLAN_FAST_DENSE = 1, 8, 16, 64  # orbx_plan_set_options flags
ORBX_PLAN_NO_TWINS = 128

EXPORTED = [
    "orbx_abi_version", "orbx_status_string", "orbx_device_count", "orbx_tables",
    "orbx_geometry_compute", "orbx_resize_tables", "orbx_extractor_create",
    "orbx_extractor_destroy", "orbx_extractor_capacity", "orbx_extract", "orbx_extractor_level",
    "orbx_extractor_set_options", "orbx_extractor_level_host", "orbx_extractor_stats",
    "orbx_boundary_record_bytes", "orbx_boundary_pack", "orbx_boundary_unpack",
    "orbx_plan_create", "orbx_plan_destroy", "orbx_plan_geometry", "orbx_plan_extract",
    "orbx_plan_check", "orbx_plan_debug_counters", "orbx_plan_fast_dense_strips", "orbx_debug_set_fast_ccap", "orbx_debug_live_resources", "orbx_debug_fail_acquire", "orbx_plan_set_options", "orbx_plan_level", "orbx_stage_count", "orbx_stage_name", "orbx_plan_set_timing",
    "orbx_plan_stage_times", "orbx_synth_frames", "orbm_search_by_bow", "orbm_search_by_bow_kf_frame",
    "orbm_descriptor_distance_batch", "orbm_plan_create", "orbm_plan_destroy",
    "orbm_plan_match_frames", "orbm_plan_set_timing", "orbm_plan_stage_times", "orbm_plan_set_options",
    "orbm_plan_fold_stats",
    "orbx_stereo_match", "orbs_plan_create", "orbs_plan_destroy", "orbs_plan_match",
    "orbs_plan_check", "orbs_plan_set_timing", "orbs_plan_stage_times",
    "orbv_vocab_load_text", "orbv_vocab_create", "orbv_vocab_destroy", "orbv_vocab_info",
    "orbv_transform", "orbv_transform_batch", "orbv_check", "orbm_search_by_projection",
    "orbm_proj_plan_create", "orbm_proj_plan_destroy", "orbm_proj_plan_search",
    "orbm_predict_scale_thresholds", "orbm_project_points", "orbm_proj_plan_project", "orbm_proj_plan_track",
    "orbm_compute_distinctive_descriptors", "orbx_undistort_keypoints", "orbx_selftest_sincos",
    "orbx_selftest_sincos_range", "orbm_search_for_triangulation", "orbm_keyframe_search",
    "orbm_search_for_initialization", "orbm_search_for_initialization_stats",
    "orbv_score", "orbv_db_create", "orbv_db_destroy", "orbv_db_add", "orbv_db_erase", "orbv_db_clear",
    "orbv_db_size", "orbv_db_query", "orbv_db_query_batch", "orbv_db_query_batch_device",
    "orbm_keyframe_project", "orbm_kf_plan_create", "orbm_kf_plan_destroy", "orbm_kf_plan_search",
    "orbm_kf_plan_project", "orbm_kf_plan_project_search",
    "orbm_pose_optimization", "orbm_pose_plan_create", "orbm_pose_plan_destroy", "orbm_pose_plan_optimize",
    "orbm_initializer_ransac", "orbm_initializer_reconstruct", "orbm_sim3_solve",
]


class Params(ctypes.Structure):
    _fields_ = [("nfeatures", ctypes.c_int), ("scale_factor", ctypes.c_float),
                ("nlevels", ctypes.c_int), ("ini_th_fast", ctypes.c_int),
                ("min_th_fast", ctypes.c_int), ("cell_guard", ctypes.c_int)]


def params(nfeatures, scale_factor, nlevels, ini_th, min_th, cell_guard="strict"):
    return Params(nfeatures, scale_factor, nlevels, ini_th, min_th,
                  1 if cell_guard in ("empty", 1, True) else 0)


class Geometry(ctypes.Structure):
    _fields_ = [("nlevels", ctypes.c_int)] + [
        (n, ctypes.c_int * 32) for n in ("width", "height", "alias", "ncols", "nrows", "wcell",
                                         "hcell", "ncells_bad", "features", "nini", "kcap_level")
    ] + [("kcap", ctypes.c_int), ("pixels", ctypes.c_longlong), ("bytes_pyr_fast", ctypes.c_longlong)]

    def level(self, name):
        return list(getattr(self, name))[:self.nlevels]


class ProjQuery(ctypes.Structure):
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("radius", ctypes.c_float),
                ("min_level", ctypes.c_int32), ("max_level", ctypes.c_int32),
                ("xr", ctypes.c_float), ("angle", ctypes.c_float)]


PROJ_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("min_level", "<i4"),
                             ("max_level", "<i4"), ("xr", "<f4"), ("angle", "<f4")])


class ProjFrame(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("uright", ctypes.c_void_p), ("occupied", ctypes.c_void_p),
                ("min_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("grid_w_inv", ctypes.c_float), ("grid_h_inv", ctypes.c_float)]


class ProjProblem(ctypes.Structure):
    _fields_ = [("frame", ProjFrame), ("q", ctypes.c_void_p), ("qdesc", ctypes.c_void_p),
                ("nq", ctypes.c_int), ("match", ctypes.c_void_p), ("nmatches", ctypes.c_void_p)]


PROJ_MAX_LEVELS = 32  # ORBX_PROJ_MAX_LEVELS
LEVEL_RULE_NEITHER, LEVEL_RULE_FORWARD, LEVEL_RULE_BACKWARD = 0, 1, 2


class ProjCamera(ctypes.Structure):  # orbx_proj_camera
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("mbf", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("max_y", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("scale_factors", ctypes.c_float * PROJ_MAX_LEVELS), ("log_scale_factor", ctypes.c_float)]


class ProjPoints(ctypes.Structure):  # orbx_proj_points
    _fields_ = [(n, ctypes.c_void_p) for n in ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist",
                                               "octave", "angle", "skip")]


class ProjParams(ctypes.Structure):  # orbx_proj_params
    _fields_ = [("th", ctypes.c_float), ("viewing_cos_limit", ctypes.c_float), ("level_rule", ctypes.c_int)]


class ProjBuildProblem(ctypes.Structure):  # orbx_proj_build_problem
    _fields_ = [("camera", ProjCamera), ("points", ProjPoints), ("npts", ctypes.c_int),
                ("q", ctypes.c_void_p), ("level", ctypes.c_void_p), ("view_cos", ctypes.c_void_p),
                ("n_in_view", ctypes.c_void_p), ("n_nonfinite", ctypes.c_void_p), ("frame", ProjFrame),
                ("qdesc", ctypes.c_void_p), ("match", ctypes.c_void_p), ("nmatches", ctypes.c_void_p)]


class PoseCamera(ctypes.Structure):  # orbx_pose_camera
    _fields_ = [("Tcw", ctypes.c_float * 12), ("fx", ctypes.c_float), ("fy", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("mbf", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("inv_level_sigma2", ctypes.c_float * PROJ_MAX_LEVELS)]


class PoseObs(ctypes.Structure):  # orbx_pose_obs
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("uright", ctypes.c_void_p),
                ("pos", ctypes.c_void_p), ("point_index", ctypes.c_void_p), ("has_point", ctypes.c_void_p),
                ("npos", ctypes.c_int)]


class PoseProblem(ctypes.Structure):  # orbx_pose_problem
    _fields_ = [("camera", PoseCamera), ("obs", PoseObs), ("Tcw_out", ctypes.c_void_p),
                ("outlier", ctypes.c_void_p), ("ninliers", ctypes.c_void_p), ("status", ctypes.c_void_p)]


POSE_MAX_N = 8192  # ORBX_POSE_MAX_N


class BowFrame(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("desc", ctypes.c_void_p), ("angle", ctypes.c_void_p),
                ("valid", ctypes.c_void_p), ("nnodes", ctypes.c_int), ("node_id", ctypes.c_void_p),
                ("node_off", ctypes.c_void_p), ("feat", ctypes.c_void_p)]


class TriFrame(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("has_mp", ctypes.c_void_p), ("nnodes", ctypes.c_int), ("node_id", ctypes.c_void_p),
                ("node_off", ctypes.c_void_p), ("feat", ctypes.c_void_p),
                ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


class KfFrame(ctypes.Structure):  # orbx_kf_frame
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("min_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("grid_w_inv", ctypes.c_float), ("grid_h_inv", ctypes.c_float)]


class KfQuery(ctypes.Structure):  # orbx_kf_query
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("radius", ctypes.c_float),
                ("level", ctypes.c_int32), ("desc", ctypes.c_int32)]


KF_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("level", "<i4"),
                           ("desc", "<i4")])
assert KF_QUERY_DTYPE.itemsize == ctypes.sizeof(KfQuery) == 20

KF_FORM_FUSE, KF_FORM_SIM3 = 1, 2  # ORBX_KF_FORM_*
KF_POINT_FIELDS = ("pos", "min_dist_inv", "max_dist_inv", "max_dist", "skip")


class KfCamera(ctypes.Structure):  # orbx_kf_camera
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("sR21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("max_y", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("scale_factors", ctypes.c_float * PROJ_MAX_LEVELS), ("log_scale_factor", ctypes.c_float)]


class KfPoints(ctypes.Structure):  # orbx_kf_points
    _fields_ = [(n, ctypes.c_void_p) for n in KF_POINT_FIELDS]


class KfProblem(ctypes.Structure):  # orbx_kf_problem
    _fields_ = [("camera", KfCamera), ("points", KfPoints), ("npts", ctypes.c_int), ("qdesc", ctypes.c_void_p),
                ("frame", KfFrame), ("q", ctypes.c_void_p), ("level", ctypes.c_void_p),
                ("n_live", ctypes.c_void_p), ("n_nonfinite", ctypes.c_void_p),
                ("best_idx", ctypes.c_void_p), ("best_dist", ctypes.c_void_p)]


class InitPair(ctypes.Structure):  # orbx_init_pair
    _fields_ = [("f1", KfFrame), ("f2", KfFrame), ("prev_matched", ctypes.c_void_p),
                ("match12", ctypes.c_void_p)]


class RansacPair(ctypes.Structure):  # orbx_ransac_pair
    _fields_ = [("n1", ctypes.c_int), ("n2", ctypes.c_int), ("keys1", ctypes.c_void_p), ("keys2", ctypes.c_void_p),
                ("match12", ctypes.c_void_p), ("sets", ctypes.c_void_p)]


# orbx_ransac_result
RANSAC_RESULT_DTYPE = np.dtype([("H21", "<f4", (3, 3)), ("F21", "<f4", (3, 3)), ("SH", "<f4"), ("SF", "<f4"),
                                ("RH", "<f4"), ("it_H", "<i4"), ("it_F", "<i4"), ("nmatch", "<i4")])


class ReconPair(ctypes.Structure):  # orbx_recon_pair
    _fields_ = [("n1", ctypes.c_int), ("n2", ctypes.c_int), ("keys1", ctypes.c_void_p), ("keys2", ctypes.c_void_p),
                ("match12", ctypes.c_void_p), ("K", ctypes.c_float * 9), ("model", ctypes.c_int32),
                ("ransac", ctypes.c_void_p), ("inliers_H", ctypes.c_void_p), ("inliers_F", ctypes.c_void_p)]


# orbx_recon_result
RECON_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("model_used", "<i4"), ("R21", "<f4", (3, 3)), ("t21", "<f4", (3,)),
                               ("best", "<i4"), ("ncand", "<i4"), ("nGood", "<i4", (8,)), ("parallax", "<f4", (8,)),
                               ("n_inliers", "<i4")])
RECON_H, RECON_F, RECON_AUTO = 0, 1, 2  # ORBX_RECON_*


class Sim3Problem(ctypes.Structure):  # orbx_sim3_problem
    _fields_ = [("ncorr", ctypes.c_int), ("pos1", ctypes.c_void_p), ("pos2", ctypes.c_void_p),
                ("sigma2_1", ctypes.c_void_p), ("sigma2_2", ctypes.c_void_p),
                ("Rcw1", ctypes.c_float * 9), ("tcw1", ctypes.c_float * 3),
                ("Rcw2", ctypes.c_float * 9), ("tcw2", ctypes.c_float * 3),
                ("K1", ctypes.c_float * 4), ("K2", ctypes.c_float * 4),  # fx fy cx cy of each keyframe
                ("nit", ctypes.c_int), ("triples", ctypes.c_void_p), ("min_inliers", ctypes.c_int),
                ("fix_scale", ctypes.c_int), ("best_in", ctypes.c_int)]


# orbx_sim3_result
SIM3_RESULT_DTYPE = np.dtype([("it_hit", "<i4"), ("it_best", "<i4"), ("n_best", "<i4"), ("ncorr", "<i4"),
                              ("R12", "<f4", (3, 3)), ("t12", "<f4", (3,)), ("s12", "<f4"),
                              ("sR21", "<f4", (3, 3)), ("t21", "<f4", (3,))])
assert SIM3_RESULT_DTYPE.itemsize == 116


# k_init_cand's list length per row and the feature limit (csrc/init_internal.h)
INIT_T, INIT_MAXN = 8, 8192

# k_kfwin_search's lanes per query and k_kfwin_grid's feature limit
# (csrc/kfwin_internal.h)
KFW_G, KFW_MAXN = 8, 8192

# k_tri_search's tile (csrc/tri_internal.h): KF1 rows per wavefront and KF2
# list entries staged in LDS at a time
TRI_ROWS, TRI_CHUNK = 64, 64

P, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
_sig = {
    "orbx_abi_version": (I, []),
    "orbx_status_string": (ctypes.c_char_p, [I]),
    "orbx_device_count": (I, []),
    "orbx_tables": (I, [P, P, P, P, P, P, P]),
    "orbx_geometry_compute": (I, [P, I, I, P]),
    "orbx_resize_tables": (I, [P, I, I, I, P, P, P, P]),
    "orbx_extractor_create": (I, [P, I, P]),
    "orbx_extractor_destroy": (I, [P]),
    "orbx_extractor_capacity": (I, [P, I, I, P]),
    "orbx_extract": (I, [P, P, I, I, SZ, P, I, P, P]),
    "orbx_extractor_level": (I, [P, I, P, SZ, P, P]),
    "orbx_extractor_set_options": (I, [P, I]),
    "orbx_extractor_level_host": (I, [P, I, P, P, P, P]),
    "orbx_extractor_stats": (I, [P, P, P]),
    "orbx_boundary_record_bytes": (SZ, [I]),
    "orbx_boundary_pack": (I, [P, P, P, I, P, P]),
    "orbx_boundary_unpack": (I, [P, I, P, P, P, P]),
    "orbx_plan_create": (I, [P, I, I, I, I, P]),
    "orbx_plan_destroy": (I, [P]),
    "orbx_plan_geometry": (I, [P, P]),
    "orbx_plan_extract": (I, [P, P, I, SZ, SZ, P, P, P, P]),
    "orbx_plan_check": (I, [P, P]),
    "orbx_plan_debug_counters": (I, [P, P]),
    "orbx_plan_fast_dense_strips": (I, [P, P]),
    "orbx_debug_set_fast_ccap": (I, [I]),
    "orbx_debug_live_resources": (I, [P]),
    "orbx_debug_fail_acquire": (I, [I]),
    "orbx_plan_set_options": (I, [P, I]),
    "orbx_plan_level": (I, [P, I, I, P, SZ, P, P, P]),
    "orbx_stage_count": (I, []),
    "orbx_stage_name": (ctypes.c_char_p, [I]),
    "orbx_plan_set_timing": (I, [P, I]),
    "orbx_plan_stage_times": (I, [P, P, P, I]),
    "orbx_synth_frames": (I, [P, I, I, SZ, I, I, I, P]),
    "orbm_search_by_bow": (I, [P, P, F, I, I, P, P]),
    "orbm_search_by_bow_kf_frame": (I, [P, P, F, I, I, P, P]),
    "orbm_search_for_triangulation": (I, [P, I, P, P, I, I, I, P, P]),
    "orbm_keyframe_search": (I, [I, P, P, P, P, I, I, P, P]),
    "orbm_search_for_initialization": (I, [I, P, I, F, I, I, P]),
    "orbm_search_for_initialization_stats": (I, [I, P, I, F, I, I, P, P]),
    "orbm_descriptor_distance_batch": (I, [P, I, P, I, P, P, I, I, P]),
    "orbm_plan_create": (I, [I, I, I, I, P]),
    "orbm_plan_destroy": (I, [P]),
    "orbm_plan_match_frames": (I, [P, I, P, P, P, P, P, P, F, I, P, P, P]),
    "orbm_plan_set_timing": (I, [P, I]),
    "orbm_plan_set_options": (I, [P, I]),
    "orbm_plan_stage_times": (I, [P, P, P, I]),
    "orbm_plan_fold_stats": (I, [P, P]),
    "orbx_stereo_match": (I, [P, P, P, P, I, P, P, I, F, F, P, P, P]),
    "orbs_plan_create": (I, [P, I, P]),
    "orbs_plan_destroy": (I, [P]),
    "orbs_plan_match": (I, [P, I, P, P, P, P, SZ, SZ, P, P, P, P, P, P, F, F, P, P, P, P]),
    "orbs_plan_check": (I, [P, P]),
    "orbs_plan_set_timing": (I, [P, I]),
    "orbs_plan_stage_times": (I, [P, P, P, I]),
    "orbv_vocab_load_text": (I, [ctypes.c_char_p, I, P]),
    "orbv_vocab_create": (I, [I, I, I, I, I, P, P, P, P, I, P]),
    "orbv_vocab_destroy": (I, [P]),
    "orbv_vocab_info": (I, [P, P, P, P, P, P, P]),
    "orbv_transform": (I, [P, P, I, I, P, P, P, P, P, P, P]),
    "orbv_transform_batch": (I, [P, I, P, P, I, I, P, P, P, P, P, P, P, P]),
    "orbv_check": (I, [P, P]),
    "orbv_score": (I, [P, P, P, I, P, P, P, I, P]),
    "orbv_db_create": (I, [P, SZ, I, P]),
    "orbv_db_destroy": (I, [P]),
    "orbv_db_add": (I, [P, ctypes.c_uint64, P, P, I]),
    "orbv_db_erase": (I, [P, ctypes.c_uint64]),
    "orbv_db_clear": (I, [P]),
    "orbv_db_size": (I, [P, P]),
    "orbv_db_query": (I, [P, P, P, I, I, P, P, P, P]),
    "orbv_db_query_batch": (I, [P, I, P, P, P, I, I, P, P, P, P]),
    "orbv_db_query_batch_device": (I, [P, I, P, P, P, I, I, I, P, P, P, P, P]),
    "orbm_search_by_projection": (I, [I, P, P, P, I, F, I, I, I, P, P]),
    "orbm_proj_plan_create": (I, [I, I, I, I, P]),
    "orbm_proj_plan_destroy": (I, [P]),
    "orbm_proj_plan_search": (I, [P, I, I, P, F, I, I, P]),
    "orbm_predict_scale_thresholds": (I, [F, I, P]),
    "orbm_project_points": (I, [I, I, P, P, P, P, I, P, P, P, P]),
    "orbm_proj_plan_project": (I, [P, I, I, P, P, P]),
    "orbm_proj_plan_track": (I, [P, I, I, P, P, F, I, I, P]),
    "orbm_keyframe_project": (I, [I, I, P, P, P, P, F, I, P, P, P]),
    "orbm_kf_plan_create": (I, [I, I, I, I, P]),
    "orbm_kf_plan_destroy": (I, [P]),
    "orbm_kf_plan_search": (I, [P, I, P, P]),
    "orbm_kf_plan_project": (I, [P, I, I, P, F, P]),
    "orbm_kf_plan_project_search": (I, [P, I, I, P, F, P]),
    "orbm_pose_optimization": (I, [I, P, P, I, P, P, P]),
    "orbm_pose_plan_create": (I, [I, I, I, P]),
    "orbm_pose_plan_destroy": (I, [P]),
    "orbm_pose_plan_optimize": (I, [P, I, P, P]),
    "orbm_initializer_ransac": (I, [I, P, I, F, I, P, P, P, P]),
    "orbm_initializer_reconstruct": (I, [I, P, F, F, I, I, P, P, P, P]),
    "orbm_sim3_solve": (I, [I, P, I, P, P, P]),
    "orbm_compute_distinctive_descriptors": (I, [P, P, I, I, P]),
    "orbx_undistort_keypoints": (I, [P, I, P, P, I, I, P]),
    "orbx_selftest_sincos": (I, [P, I, P, P]),
    "orbx_selftest_sincos_range": (I, [ctypes.c_uint32, I, P, I]),
}
for _n, (_r, _a) in _sig.items():
    _f = getattr(_lib, _n)
    _f.restype = _r
    _f.argtypes = _a


def lib():
    return _lib


class OrbxError(RuntimeError):
    def __init__(self, code, what=""):
        msg = _lib.orbx_status_string(code).decode()
        super().__init__("%s: %s (%d)" % (what, msg, code) if what else "%s (%d)" % (msg, code))
        self.code = code


def _check(rc, what=""):
    if rc != OK:
        raise OrbxError(rc, what)
    return rc


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dptr(t):
    """device pointer of a cuda tensor, NULL for None"""
    return None if t is None else t.data_ptr()


def _proj_frame(fr):
    """ProjFrame of a dict of cuda tensors (keys, desc, uright | None, occupied | None) and the grid floats"""
    return ProjFrame(fr["keys"].shape[0], _dptr(fr["keys"]), _dptr(fr["desc"]), _dptr(fr.get("uright")),
                     _dptr(fr.get("occupied")), fr["min_x"], fr["min_y"], fr["grid_w_inv"], fr["grid_h_inv"])


def device_count():
    return _lib.orbx_device_count()


def stage_names():
    return [_lib.orbx_stage_name(i).decode() for i in range(_lib.orbx_stage_count())]


# --------------------------------------------------------------------------- host-only tables
def tables(prm):
    L = prm.nlevels
    s, inv, s2, inv2 = (np.zeros(L, np.float32) for _ in range(4))
    fpl = np.zeros(L, np.int32)
    umax = np.zeros(16, np.int32)
    _check(_lib.orbx_tables(ctypes.byref(prm), _p(s), _p(inv), _p(s2), _p(inv2), _p(fpl), _p(umax)))
    return dict(scale=s, inv_scale=inv, sigma2=s2, inv_sigma2=inv2, features_per_level=fpl,
                umax=umax)


def geometry(prm, width, height):
    g = Geometry()
    _check(_lib.orbx_geometry_compute(ctypes.byref(prm), width, height, ctypes.byref(g)), "geometry")
    return g


def resize_tables(prm, width, height, level):
    g = geometry(prm, width, height)
    w, h = g.width[level], g.height[level]
    xofs = np.zeros(w, np.int32)
    alpha = np.zeros(2 * w, np.int16)
    yofs = np.zeros(h, np.int32)
    beta = np.zeros(2 * h, np.int16)
    _check(_lib.orbx_resize_tables(ctypes.byref(prm), width, height, level, _p(xofs), _p(alpha),
                                   _p(yofs), _p(beta)))
    return xofs, alpha.reshape(w, 2), yofs, beta.reshape(h, 2)


# --------------------------------------------------------------------------- ORBextractor
class Extractor:
    """ORB_SLAM2::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)."""

    def __init__(self, nfeatures, scale_factor, nlevels, ini_th, min_th, cell_guard="strict",
                 device=0):
        self.params = params(nfeatures, scale_factor, nlevels, ini_th, min_th, cell_guard)
        self._t = tables(self.params)
        h = ctypes.c_void_p()
        _check(_lib.orbx_extractor_create(ctypes.byref(self.params), device, ctypes.byref(h)),
               "orbx_extractor_create")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbx_extractor_destroy(self._h)
            self._h = None

    # getters (ORBextractor.h:43-63)
    def GetLevels(self):
        return self.params.nlevels

    def GetScaleFactor(self):
        return self.params.scale_factor

    def GetScaleFactors(self):
        return self._t["scale"].tolist()

    def GetInverseScaleFactors(self):
        return self._t["inv_scale"].tolist()

    def GetScaleSigmaSquares(self):
        return self._t["sigma2"].tolist()

    def GetInverseScaleSigmaSquares(self):
        return self._t["inv_sigma2"].tolist()

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors) -> (keypoints, descriptors)."""
        return self.extract(image)

    def extract(self, image):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.ndim != 2:
            raise OrbxError(ERR_ARG, "CV_8UC1 image expected")
        h, w = img.shape
        cap = ctypes.c_int(0)
        _check(_lib.orbx_extractor_capacity(self._h, w, h, ctypes.byref(cap)), "capacity")
        kps = np.zeros(max(cap.value, 1), KEYPOINT_DTYPE)
        desc = np.zeros((max(cap.value, 1), 32), np.uint8)
        n = ctypes.c_int(0)
        _check(_lib.orbx_extract(self._h, _p(img), w, h, w, _p(kps), cap.value, _p(desc),
                                 ctypes.byref(n)), "orbx_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def level(self, l):
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(_lib.orbx_extractor_level(self._h, l, None, 0, ctypes.byref(w), ctypes.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(_lib.orbx_extractor_level(self._h, l, _p(out), w.value, None, None))
        return out

    def set_options(self, pyramid_to_host=False, pinned_h2d=False):
        """ORBX_EXTRACTOR_* options (include/orbx.h)"""
        _check(_lib.orbx_extractor_set_options(self._h, (1 if pyramid_to_host else 0)
                                               | (2 if pinned_h2d else 0)), "orbx_extractor_set_options")

    def level_host(self, l):
        """copy of the host pyramid level the last extract() brought back
        (pyramid_to_host option)"""
        d, st = ctypes.c_void_p(), ctypes.c_size_t()
        w, h = ctypes.c_int(), ctypes.c_int()
        _check(_lib.orbx_extractor_level_host(self._h, l, ctypes.byref(d), ctypes.byref(st),
                                              ctypes.byref(w), ctypes.byref(h)), "orbx_extractor_level_host")
        buf = (ctypes.c_uint8 * (st.value * (h.value - 1) + w.value)).from_address(d.value)
        a = np.frombuffer(buf, np.uint8)
        return np.lib.stride_tricks.as_strided(a, (h.value, w.value), (st.value, 1)).copy()

    def stats(self):
        c, r = ctypes.c_longlong(), ctypes.c_longlong()
        _check(_lib.orbx_extractor_stats(self._h, ctypes.byref(c), ctypes.byref(r)))
        return {"calls": c.value, "refetches": r.value}


# --------------------------------------------------------------------------- stereo
def compute_stereo_matches(left, right, kps_l, desc_l, kps_r, desc_r, mb, mbf):
    """Frame::ComputeStereoMatches (Frame.cc:446-620) for the pair whose images
    were the last extract() of Extractor `left` and `right` (their pyramids
    stay on the device).  Returns (mvuRight f32[N], mvDepth f32[N], nmatches)."""
    kl = np.ascontiguousarray(kps_l, KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kps_r, KEYPOINT_DTYPE)
    dl = np.ascontiguousarray(desc_l, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(desc_r, np.uint8).reshape(-1, 32)
    ur = np.full(max(len(kl), 1), -1, np.float32)
    dep = np.full(max(len(kl), 1), -1, np.float32)
    nm = ctypes.c_int(0)
    _check(_lib.orbx_stereo_match(left._h, right._h, _p(kl), _p(dl), len(kl), _p(kr), _p(dr),
                                  len(kr), float(mb), float(mbf), _p(ur), _p(dep),
                                  ctypes.byref(nm)), "orbx_stereo_match")
    return ur[:len(kl)].copy(), dep[:len(kl)].copy(), nm.value


# --------------------------------------------------------------------------- DBoW2 vocabulary
class Vocabulary:
    """DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (ORBVocabulary) on
    the device: loadFromTextFile + transform (TemplatedVocabulary.h:1126-1424)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load_text(cls, path, device=0):
        h = ctypes.c_void_p()
        _check(_lib.orbv_vocab_load_text(os.fsencode(path), device, ctypes.byref(h)),
               "orbv_vocab_load_text")
        return cls(h)

    @classmethod
    def from_records(cls, voc, scoring=0, weighting=0, device=0):
        parent = np.ascontiguousarray(voc["parent"], np.int32)
        leaf = np.ascontiguousarray(voc["is_leaf"], np.int32)
        desc = np.ascontiguousarray(voc["desc"], np.uint8)
        w = np.ascontiguousarray(voc["weight"], np.float64)
        h = ctypes.c_void_p()
        _check(_lib.orbv_vocab_create(voc["k"], voc["L"], scoring, weighting, len(parent),
                                      _p(parent), _p(leaf), _p(desc), _p(w), device,
                                      ctypes.byref(h)), "orbv_vocab_create")
        return cls(h)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbv_vocab_destroy(self._h)
            self._h = None

    def info(self):
        v = [ctypes.c_int() for _ in range(6)]
        _check(_lib.orbv_vocab_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("k", "L", "scoring", "weighting", "nnodes", "nwords"),
                        [x.value for x in v]))

    def transform(self, desc, levelsup=4):
        """-> (BowVector (word ids u32, values f64), FeatureVector dict(node_id, off, feat))"""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        m = max(n, 1)
        bw, bv = np.zeros(m, np.uint32), np.zeros(m, np.float64)
        fn, fo, ff = np.zeros(m, np.uint32), np.zeros(m + 1, np.uint32), np.zeros(m, np.uint32)
        nb, nf = ctypes.c_int(), ctypes.c_int()
        _check(_lib.orbv_transform(self._h, _p(d), n, levelsup, _p(bw), _p(bv), ctypes.byref(nb),
                                   _p(fn), _p(fo), _p(ff), ctypes.byref(nf)), "orbv_transform")
        nfe = int(fo[nf.value])
        return ((bw[:nb.value].copy(), bv[:nb.value].copy()),
                dict(node_id=fn[:nf.value].copy(), off=fo[:nf.value + 1].copy(),
                     feat=ff[:nfe].copy()))

    def transform_batch(self, desc, counts, levelsup=4, stream=None):
        """Device form over Plan outputs: desc cuda u8 [B, kcap, 32], counts i32 [B].
        Async; returns dict of cuda tensors (bow_word, bow_value, nbow, fv_node,
        fv_off, fv_feat, nfv), rows per frame as in orbv_transform."""
        import torch
        B, kcap = desc.shape[0], desc.shape[1]
        dev = desc.device
        o = dict(bow_word=torch.empty((B, kcap), dtype=torch.int32, device=dev),
                 bow_value=torch.empty((B, kcap), dtype=torch.float64, device=dev),
                 nbow=torch.empty(B, dtype=torch.int32, device=dev),
                 fv_node=torch.empty((B, kcap), dtype=torch.int32, device=dev),
                 fv_off=torch.empty((B, kcap + 1), dtype=torch.int32, device=dev),
                 fv_feat=torch.empty((B, kcap), dtype=torch.int32, device=dev),
                 nfv=torch.empty(B, dtype=torch.int32, device=dev))
        _check(_lib.orbv_transform_batch(self._h, B, desc.data_ptr(), counts.data_ptr(), kcap,
                                         levelsup, o["bow_word"].data_ptr(),
                                         o["bow_value"].data_ptr(), o["nbow"].data_ptr(),
                                         o["fv_node"].data_ptr(), o["fv_off"].data_ptr(),
                                         o["fv_feat"].data_ptr(), o["nfv"].data_ptr(),
                                         _stream_handle(stream)), "orbv_transform_batch")
        return o

    def check(self, stream=None):
        _check(_lib.orbv_check(self._h, _stream_handle(stream)), "orbv_check")

    def score(self, a, list_of_b):
        """TemplatedVocabulary::score(a, b) for every b of the list, with the
        vocabulary's scoring: BowVectors as (words u32 ascending, values f64)
        -> f64[len(list_of_b)]"""
        aw, av = _bow_vector(a)
        bs = [_bow_vector(b) for b in list_of_b]
        off = np.zeros(len(bs) + 1, np.uint32)
        off[1:] = np.cumsum([len(w) for w, _ in bs])
        bw = np.concatenate([w for w, _ in bs]) if bs else np.zeros(0, np.uint32)
        bv = np.concatenate([v for _, v in bs]) if bs else np.zeros(0, np.float64)
        out = np.zeros(len(bs), np.float64)
        _check(_lib.orbv_score(self._h, _p(aw), _p(av), len(aw), _p(off), _p(bw), _p(bv), len(bs), _p(out)),
               "orbv_score")
        return out


def _bow_vector(b):
    w = np.ascontiguousarray(b[0], np.uint32).reshape(-1)
    v = np.ascontiguousarray(b[1], np.float64).reshape(-1)
    if len(w) != len(v):
        raise OrbxError(ERR_ARG, "BowVector: one value per word expected")
    return w, v


class KeyFrameDatabase:
    """The reference's KeyFrameDatabase inverted file on the device
    (src/KeyFrameDatabase.cc): stored BowVectors keyed by keyframe id; query()
    is the word walk of DetectLoopCandidates / DetectRelocalizationCandidates
    with the scores."""

    def __init__(self, vocabulary, reserve_words=0, device=0):
        h = ctypes.c_void_p()
        _check(_lib.orbv_db_create(vocabulary._h, reserve_words, device, ctypes.byref(h)), "orbv_db_create")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbv_db_destroy(self._h)
            self._h = None

    def add(self, kf_id, bow):
        w, v = _bow_vector(bow)
        _check(_lib.orbv_db_add(self._h, kf_id, _p(w), _p(v), len(w)), "orbv_db_add")

    def erase(self, kf_id):
        _check(_lib.orbv_db_erase(self._h, kf_id), "orbv_db_erase")

    def clear(self):
        _check(_lib.orbv_db_clear(self._h), "orbv_db_clear")

    def size(self):
        n = ctypes.c_int()
        _check(_lib.orbv_db_size(self._h, ctypes.byref(n)), "orbv_db_size")
        return n.value

    def query(self, bow):
        """-> (ids u64, ncommon i32, score f64) of every stored keyframe sharing
        a word with `bow`, in the order of the reference's lKFsSharingWords"""
        w, v = _bow_vector(bow)
        cap = max(self.size(), 1)
        ids, nc, sc = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        n = ctypes.c_int()
        _check(_lib.orbv_db_query(self._h, _p(w), _p(v), len(w), cap, _p(ids), _p(nc), _p(sc), ctypes.byref(n)),
               "orbv_db_query")
        return ids[:n.value].copy(), nc[:n.value].copy(), sc[:n.value].copy()

    def query_batch(self, bows, gated=False):
        """query() for every BowVector of the list in one call -> a list of
        (ids u64, ncommon i32, score f64); gated: each list keeps only the
        entries with ncommon > int(max ncommon * 0.8f), order kept"""
        qs = [_bow_vector(b) for b in bows]
        off = np.zeros(len(qs) + 1, np.uint32)
        off[1:] = np.cumsum([len(w) for w, _ in qs])
        qw = np.concatenate([w for w, _ in qs]) if qs else np.zeros(0, np.uint32)
        qv = np.concatenate([v for _, v in qs]) if qs else np.zeros(0, np.float64)
        flags = ORBV_QUERY_GATED if gated else 0
        out = np.zeros(len(qs) + 1, np.uint32)
        cap = max(self.size(), 1)
        for attempt in range(2):  # once more with the total the call asks for
            ids, nc, sc = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
            rc = _lib.orbv_db_query_batch(self._h, len(qs), _p(off), _p(qw), _p(qv), flags, cap, _p(out), _p(ids),
                                          _p(nc), _p(sc))
            if rc != ERR_CAPACITY or attempt:
                break
            cap = int(out[-1])
        _check(rc, "orbv_db_query_batch")
        return [(ids[a:b].copy(), nc[a:b].copy(), sc[a:b].copy()) for a, b in zip(out[:-1].tolist(), out[1:].tolist())]

    def query_batch_device(self, word, value, n, cap, gated=False, stream=None):
        """Device form over Vocabulary.transform_batch outputs: word cuda i32
        [B, qstride], value cuda f64 [B, qstride], n cuda i32 [B].  Async on
        `stream`; returns dict of cuda tensors kf_id i64 [B, cap], ncommon i32
        [B, cap], score f64 [B, cap] (for L2_NORM the sum before the closing
        sqrt step) and nsharing i32 [B]: row q's first min(nsharing[q], cap)
        entries are query()'s list, nsharing[q] == -1 for n[q] > qstride.  The
        words are not checked."""
        import torch
        B, qstride = word.shape[0], word.shape[1]
        dev = word.device
        o = dict(kf_id=torch.empty((B, cap), dtype=torch.int64, device=dev),
                 ncommon=torch.empty((B, cap), dtype=torch.int32, device=dev),
                 score=torch.empty((B, cap), dtype=torch.float64, device=dev),
                 nsharing=torch.empty(B, dtype=torch.int32, device=dev))
        self.query_batch_device_into(word, value, n, o, gated, stream)
        return o

    def query_batch_device_into(self, word, value, n, out, gated=False, stream=None):
        """query_batch_device into the tensors of an earlier call's dict"""
        B, qstride = word.shape[0], word.shape[1]
        cap = out["kf_id"].shape[1]
        _check(_lib.orbv_db_query_batch_device(self._h, B, word.data_ptr(), value.data_ptr(), n.data_ptr(), qstride,
                                               ORBV_QUERY_GATED if gated else 0, cap, out["kf_id"].data_ptr(),
                                               out["ncommon"].data_ptr(), out["score"].data_ptr(),
                                               out["nsharing"].data_ptr(), _stream_handle(stream)),
               "orbv_db_query_batch_device")
        return out


# --------------------------------------------------------------------------- ORBmatcher
def _bow_struct(k, keep):
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    ang = np.ascontiguousarray(k["angle"], np.float32)
    valid = None if k.get("valid") is None else np.ascontiguousarray(k["valid"], np.uint8)
    nid = np.ascontiguousarray(k["node_id"], np.uint32)
    off = np.ascontiguousarray(k["off"], np.uint32)
    feat = np.ascontiguousarray(k["feat"], np.uint32)
    keep.extend([desc, ang, valid, nid, off, feat])
    return BowFrame(len(desc), _p(desc), _p(ang), _p(valid), len(nid), _p(nid), _p(off), _p(feat))


def search_by_bow(kf1, kf2, nnratio=0.6, check_ori=True, device=0):
    """SearchByBoW(KF1, KF2): returns (match12 int32[N1], nmatches)."""
    keep = []
    b1, b2 = _bow_struct(kf1, keep), _bow_struct(kf2, keep)
    m = np.full(max(b1.n, 1), -1, np.int32)
    nm = ctypes.c_int(0)
    _check(_lib.orbm_search_by_bow(ctypes.byref(b1), ctypes.byref(b2), float(nnratio),
                                   1 if check_ori else 0, device, _p(m), ctypes.byref(nm)),
           "orbm_search_by_bow")
    return m[:b1.n].copy(), nm.value


def search_by_bow_kf_frame(kf, fr, nnratio=0.6, check_ori=True, device=0):
    """Upstream ORB-SLAM2's SearchByBoW(KF, Frame) (bow_kf_frame=full; the
    reference ships a stub): returns (match_f int32[F.N], nmatches)."""
    keep = []
    b1, b2 = _bow_struct(kf, keep), _bow_struct(fr, keep)
    m = np.full(max(b2.n, 1), -1, np.int32)
    nm = ctypes.c_int(0)
    _check(_lib.orbm_search_by_bow_kf_frame(ctypes.byref(b1), ctypes.byref(b2), float(nnratio),
                                            1 if check_ori else 0, device, _p(m), ctypes.byref(nm)),
           "orbm_search_by_bow_kf_frame")
    return m[:b2.n].copy(), nm.value


def tri_struct(k, keep):
    """orbx_tri_frame of dict(keys, desc, has_mp|None, node_id, off, feat,
    level_sigma2|None); the arrays it points into are appended to keep."""
    keys = np.ascontiguousarray(k["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    mp = None if k.get("has_mp") is None else np.ascontiguousarray(k["has_mp"], np.uint8)
    nid = np.ascontiguousarray(k["node_id"], np.uint32)
    off = np.ascontiguousarray(k["off"], np.uint32)
    feat = np.ascontiguousarray(k["feat"], np.uint32)
    s2 = None if k.get("level_sigma2") is None else np.ascontiguousarray(k["level_sigma2"], np.float32)
    keep.extend([keys, desc, mp, nid, off, feat, s2])
    return TriFrame(len(keys), _p(keys), _p(desc), _p(mp), len(nid), _p(nid), _p(off), _p(feat),
                    _p(s2), 0 if s2 is None else len(s2))


def search_for_triangulation(kf1, kf2_list, F12_list, only_stereo=False, check_ori=True, device=0):
    """ORBmatcher::SearchForTriangulation(KF1, KF2, F12, ..) for every KF2 of
    kf2_list in one batched call (the neighbour loop of CreateNewMapPoints).
    Frames are dicts (tri_struct); F12_list holds one 3x3 float32 matrix per
    KF2.  Returns (match12 int32[len(kf2_list), N1], nmatches int32[len(kf2_list)]);
    vMatchedPairs of problem p = [(i, match12[p, i]) for i where match12[p, i] >= 0]."""
    keep = []
    b1 = tri_struct(kf1, keep)
    nk = len(kf2_list)
    arr = (TriFrame * max(nk, 1))()
    for p, k in enumerate(kf2_list):
        arr[p] = tri_struct(k, keep)
    F12 = np.ascontiguousarray(np.asarray(F12_list, np.float32).reshape(-1, 9))
    if len(F12) != nk:
        raise OrbxError(ERR_ARG, "one F12 per KF2 expected")
    m = np.full(max(nk * b1.n, 1), -1, np.int32)
    nm = np.zeros(max(nk, 1), np.int32)
    _check(_lib.orbm_search_for_triangulation(ctypes.byref(b1), nk, ctypes.cast(arr, ctypes.c_void_p),
                                              _p(F12), 1 if only_stereo else 0,
                                              1 if check_ori else 0, device, _p(m), _p(nm)),
           "orbm_search_for_triangulation")
    return m[:nk * b1.n].reshape(nk, b1.n).copy(), nm[:nk].copy()


def kf_struct(k, keep):
    """orbx_kf_frame of dict(keys, desc, min_x, min_y, grid_w_inv, grid_h_inv);
    the arrays it points into are appended to keep."""
    keys = np.ascontiguousarray(k["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    keep.extend([keys, desc])
    return KfFrame(len(keys), _p(keys), _p(desc), k["min_x"], k["min_y"], k["grid_w_inv"],
                   k["grid_h_inv"])


def keyframe_search(kfs, queries, qdesc, device=0):
    """The search ORBmatcher::Fuse (both forms) and SearchBySim3 share
    (orbm_keyframe_search), batched: kfs[p] is a keyframe dict (kf_struct),
    queries[p] its KF_QUERY_DTYPE array, qdesc the descriptor pool
    (uint8[npool, 32]) the queries' desc rows index.  Returns a list of
    (best_idx int32[nq_p], best_dist int32[nq_p]) per problem."""
    if len(kfs) != len(queries):
        raise OrbxError(ERR_ARG, "one query array per keyframe expected")
    keep = []
    nprob = len(kfs)
    arr = (KfFrame * max(nprob, 1))()
    for p, k in enumerate(kfs):
        arr[p] = kf_struct(k, keep)
    qs = [np.ascontiguousarray(q, KF_QUERY_DTYPE).reshape(-1) for q in queries]
    qoff = np.zeros(nprob + 1, np.int32)
    qoff[1:] = np.cumsum([len(q) for q in qs])
    q = np.concatenate(qs) if qs else np.zeros(0, KF_QUERY_DTYPE)
    q = np.ascontiguousarray(q, KF_QUERY_DTYPE)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    nq = int(qoff[-1])
    bi = np.full(max(nq, 1), -7, np.int32)
    bd = np.full(max(nq, 1), -7, np.int32)
    _check(_lib.orbm_keyframe_search(nprob, ctypes.cast(arr, ctypes.c_void_p), _p(q), _p(qoff), _p(qd),
                                     len(qd), device, _p(bi), _p(bd)), "orbm_keyframe_search")
    return [(bi[qoff[p]:qoff[p + 1]].copy(), bd[qoff[p]:qoff[p + 1]].copy()) for p in range(nprob)]


def init_pair_struct(pair, keep):
    """orbx_init_pair of dict(f1, f2, prev_matched, match12): f1 / f2 are frame
    dicts (kf_struct; f1's grid constants are not read and may be absent),
    prev_matched float32[n1, 2] and match12 int32[n1].  Both arrays are copied
    (the call writes into the copies), appended to keep and returned."""
    f1 = dict(min_x=0.0, min_y=0.0, grid_w_inv=0.0, grid_h_inv=0.0)
    f1.update(pair["f1"])
    a, b = kf_struct(f1, keep), kf_struct(pair["f2"], keep)
    prev = np.array(pair["prev_matched"], np.float32).reshape(-1, 2)
    m12 = np.array(pair["match12"], np.int32).reshape(-1)
    if len(prev) != a.n or len(m12) != a.n:
        raise OrbxError(ERR_ARG, "prev_matched and match12 need one row per F1 feature")
    keep.extend([prev, m12])
    return InitPair(a, b, _p(prev), _p(m12)), prev, m12


def search_for_initialization(pairs, window_size=100, nnratio=0.9, check_ori=True, device=0, stats=False):
    """ORBmatcher::SearchForInitialization (orbm_search_for_initialization),
    batched over independent pairs (init_pair_struct dicts): one upload, one
    set of launches, one download.  Returns per pair (match12 int32[n1],
    prev_matched float32[n1, 2], nmatches), the inputs left untouched; hand
    match12 and prev_matched back in for the next frame, as Tracking keeps
    mvIniMatches and mvbPrevMatched.  stats=True appends the number of rows
    whose walk step scanned its window again."""
    keep, out = [], []
    npair = len(pairs)
    arr = (InitPair * max(npair, 1))()
    for p, pair in enumerate(pairs):
        arr[p], prev, m12 = init_pair_struct(pair, keep)
        out.append((m12, prev))
    nm = np.zeros(max(npair, 1), np.int32)
    resc = np.zeros(max(npair, 1), np.int32)
    args = (npair, ctypes.cast(arr, ctypes.c_void_p), int(window_size), float(nnratio), 1 if check_ori else 0,
            device, _p(nm))
    if stats:
        _check(_lib.orbm_search_for_initialization_stats(*args, _p(resc)), "orbm_search_for_initialization")
        return [(m, pv, int(nm[p]), int(resc[p])) for p, (m, pv) in enumerate(out)]
    _check(_lib.orbm_search_for_initialization(*args), "orbm_search_for_initialization")
    return [(m, pv, int(nm[p])) for p, (m, pv) in enumerate(out)]


def initializer_ransac(pairs, nit, sigma=1.0, device=0):
    """Initializer::FindHomography / FindFundamental (orbm_initializer_ransac),
    batched over pairs: dict(keys1 KEYPOINT_DTYPE[n1], keys2 KEYPOINT_DTYPE[n2],
    match12 int32[n1] as search_for_initialization returns it, sets int32[nit,
    8] indices into the match list, the rows with match12 >= 0 in ascending
    order).  Returns per pair dict(H21, F21 float32[3, 3], SH, SF, RH float32,
    it_H, it_F (-1: no winner, the matrix zero), nmatch, inliers_H, inliers_F
    uint8[nmatch])."""
    npair = len(pairs)
    arr = (RansacPair * max(npair, 1))()
    keep, off = [], [0]
    for p, pair in enumerate(pairs):
        k1 = np.ascontiguousarray(pair["keys1"], KEYPOINT_DTYPE).reshape(-1)
        k2 = np.ascontiguousarray(pair["keys2"], KEYPOINT_DTYPE).reshape(-1)
        m12 = np.ascontiguousarray(pair["match12"], np.int32).reshape(-1)
        sets = np.ascontiguousarray(pair["sets"], np.int32).reshape(-1)
        if len(m12) != len(k1) or len(sets) < 8 * nit:
            raise OrbxError(ERR_ARG, "initializer_ransac: match12 needs a row per key of frame 1, sets 8 per iteration")
        keep.append((k1, k2, m12, sets))
        arr[p] = RansacPair(len(k1), len(k2), _p(k1), _p(k2), _p(m12), _p(sets))
        off.append(off[-1] + int((m12 >= 0).sum()))
    res = np.zeros(max(npair, 1), RANSAC_RESULT_DTYPE)
    inl_off = np.array(off, np.int32)
    inl_h = np.zeros(max(off[-1], 1), np.uint8)
    inl_f = np.zeros(max(off[-1], 1), np.uint8)
    _check(_lib.orbm_initializer_ransac(npair, ctypes.cast(arr, ctypes.c_void_p), int(nit), float(sigma), device,
                                        _p(res), _p(inl_h), _p(inl_f), _p(inl_off)), "orbm_initializer_ransac")
    out = []
    for p in range(npair):
        r = res[p]
        out.append(dict(H21=r["H21"].copy(), F21=r["F21"].copy(), SH=r["SH"], SF=r["SF"], RH=r["RH"],
                        it_H=int(r["it_H"]), it_F=int(r["it_F"]), nmatch=int(r["nmatch"]),
                        inliers_H=inl_h[off[p]:off[p + 1]].copy(), inliers_F=inl_f[off[p]:off[p + 1]].copy()))
    return out


def sim3_problem(pr, keep):
    """Sim3Problem of a dict as sim3_solve takes it; the arrays it points to are
    appended to `keep`"""
    pos1 = np.ascontiguousarray(pr["pos1"], np.float32).reshape(-1, 3)
    pos2 = np.ascontiguousarray(pr["pos2"], np.float32).reshape(-1, 3)
    s1 = np.ascontiguousarray(pr["sigma2_1"], np.float32).reshape(-1)
    s2 = np.ascontiguousarray(pr["sigma2_2"], np.float32).reshape(-1)
    tri = np.ascontiguousarray(pr["triples"], np.int32).reshape(-1, 3)
    n = len(pos1)
    nit = int(pr.get("nit", len(tri)))
    if not (len(pos2) == len(s1) == len(s2) == n) or len(tri) < nit:
        raise OrbxError(ERR_ARG, "sim3_solve: pos2, sigma2_1 and sigma2_2 need a row per correspondence, triples one per iteration")
    keep.append((pos1, pos2, s1, s2, tri))
    vec = lambda k, m: (ctypes.c_float * m)(*np.asarray(pr[k], np.float32).reshape(m))
    return Sim3Problem(n, _p(pos1), _p(pos2), _p(s1), _p(s2), vec("Rcw1", 9), vec("tcw1", 3), vec("Rcw2", 9),
                       vec("tcw2", 3), vec("K1", 4), vec("K2", 4), nit, _p(tri), int(pr["min_inliers"]),
                       1 if pr["fix_scale"] else 0, int(pr.get("best_in", 0)))


def sim3_solve(problems, device=0):
    """Sim3Solver's constructor values and iterate (orbm_sim3_solve), batched
    over solvers: dict(pos1, pos2 float32[ncorr, 3] world positions of the
    matched map points, sigma2_1, sigma2_2 float32[ncorr], Rcw1, tcw1, Rcw2, tcw2,
    K1, K2 = (fx, fy, cx, cy), triples int32[nit, 3] indices into the
    correspondences, min_inliers, fix_scale, best_in = 0, nit = len(triples)).
    Returns per problem dict(it_hit, it_best (-1: none), n_best, ncorr, R12
    float32[3, 3], t12 float32[3], s12, sR21 float32[3, 3], t21 float32[3] as
    orbx_kf_camera takes them, inliers uint8[ncorr])."""
    nprob = len(problems)
    arr = (Sim3Problem * max(nprob, 1))()
    keep, off = [], [0]
    for p, pr in enumerate(problems):
        arr[p] = sim3_problem(pr, keep)
        off.append(off[-1] + arr[p].ncorr)
    res = np.zeros(max(nprob, 1), SIM3_RESULT_DTYPE)
    inl_off = np.array(off, np.int32)
    inl = np.zeros(max(off[-1], 1), np.uint8)
    _check(_lib.orbm_sim3_solve(nprob, ctypes.cast(arr, ctypes.c_void_p), device, _p(res), _p(inl), _p(inl_off)),
           "orbm_sim3_solve")
    out = []
    for p in range(nprob):
        r = res[p]
        d = {k: (r[k].copy() if r[k].shape else (int(r[k]) if k != "s12" else r[k])) for k in SIM3_RESULT_DTYPE.names}
        d["inliers"] = inl[off[p]:off[p + 1]].copy()
        out.append(d)
    return out


def ransac_record(r):
    """one orbx_ransac_result record from a dict as initializer_ransac returns it
    (or from a RANSAC_RESULT_DTYPE record, passed through)"""
    if isinstance(r, np.ndarray) or isinstance(r, np.void):
        return np.ascontiguousarray(r, RANSAC_RESULT_DTYPE).reshape(())
    rec = np.zeros((), RANSAC_RESULT_DTYPE)
    for k in RANSAC_RESULT_DTYPE.names:
        rec[k] = r[k]
    return rec


def initializer_reconstruct(pairs, sigma=1.0, min_parallax=1.0, min_triangulated=50, device=0):
    """Initializer::ReconstructH / ReconstructF (orbm_initializer_reconstruct),
    batched over pairs: dict(keys1 KEYPOINT_DTYPE[n1], keys2 KEYPOINT_DTYPE[n2],
    match12 int32[n1], K float32[3, 3], model RECON_H / RECON_F / RECON_AUTO
    (default AUTO: H when RH > 0.40), ransac: the pair's result of
    initializer_ransac (its dict, or a RANSAC_RESULT_DTYPE record), inliers_H,
    inliers_F uint8[nmatch]; under a forced model the other may be None or
    missing; a dict ransac supplies them when they are not given).  Returns per
    pair dict(ok, model_used, R21 float32[3, 3], t21 float32[3], best, ncand,
    nGood int32[8], parallax float32[8], n_inliers, P3D float32[n1, 3],
    triangulated uint8[n1]); R21, t21, P3D and triangulated are zero when not
    ok."""
    npair = len(pairs)
    arr = (ReconPair * max(npair, 1))()
    keep, off = [], [0]
    for p, pair in enumerate(pairs):
        k1 = np.ascontiguousarray(pair["keys1"], KEYPOINT_DTYPE).reshape(-1)
        k2 = np.ascontiguousarray(pair["keys2"], KEYPOINT_DTYPE).reshape(-1)
        m12 = np.ascontiguousarray(pair["match12"], np.int32).reshape(-1)
        K = np.ascontiguousarray(pair["K"], np.float32).reshape(-1)
        if len(m12) != len(k1) or len(K) != 9:
            raise OrbxError(ERR_ARG, "initializer_reconstruct: match12 needs a row per key of frame 1, K nine entries")
        rs = pair["ransac"]
        rec = ransac_record(rs)
        nm = int((m12 >= 0).sum())
        fl = []
        for name in ("inliers_H", "inliers_F"):
            f = pair.get(name)
            if f is None and isinstance(rs, dict):
                f = rs.get(name)
            if f is not None:
                f = np.ascontiguousarray(f, np.uint8).reshape(-1)
                if len(f) < nm:
                    raise OrbxError(ERR_ARG, "initializer_reconstruct: a flag per entry of the match list")
            fl.append(f)
        keep.append((k1, k2, m12, rec, fl))
        arr[p] = ReconPair(len(k1), len(k2), _p(k1), _p(k2), _p(m12), (ctypes.c_float * 9)(*K.tolist()),
                           int(pair.get("model", RECON_AUTO)), _p(rec), None if fl[0] is None else _p(fl[0]),
                           None if fl[1] is None else _p(fl[1]))
        off.append(off[-1] + len(k1))
    res = np.zeros(max(npair, 1), RECON_RESULT_DTYPE)
    key_off = np.array(off, np.int32)
    p3d = np.zeros((max(off[-1], 1), 3), np.float32)
    tri = np.zeros(max(off[-1], 1), np.uint8)
    _check(_lib.orbm_initializer_reconstruct(npair, ctypes.cast(arr, ctypes.c_void_p), float(sigma),
                                             float(min_parallax), int(min_triangulated), device, _p(res), _p(p3d),
                                             _p(tri), _p(key_off)), "orbm_initializer_reconstruct")
    out = []
    for p in range(npair):
        r = res[p]
        out.append(dict(ok=int(r["ok"]), model_used=int(r["model_used"]), R21=r["R21"].copy(), t21=r["t21"].copy(),
                        best=int(r["best"]), ncand=int(r["ncand"]), nGood=r["nGood"].copy(),
                        parallax=r["parallax"].copy(), n_inliers=int(r["n_inliers"]),
                        P3D=p3d[off[p]:off[p + 1]].copy(), triangulated=tri[off[p]:off[p + 1]].copy()))
    return out


def descriptor_distance_batch(a, b, ia, ib, device=0):
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32)
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    out = np.zeros(len(ia), np.int32)
    _check(_lib.orbm_descriptor_distance_batch(_p(a), len(a), _p(b), len(b), _p(ia), _p(ib),
                                               len(ia), device, _p(out)))
    return out


def search_by_projection(mode, frame, queries, qdesc, nnratio=0.6, th_dist=100, check_ori=True,
                         device=0):
    """ORBmatcher::SearchByProjection in query form (orbm_search_by_projection).
    frame = dict(keys, desc, uright|None, occupied|None, min_x, min_y, grid_w_inv,
    grid_h_inv); queries = PROJ_QUERY_DTYPE array.  Returns (match int32[n], nmatches)."""
    keys = np.ascontiguousarray(frame["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(frame["desc"], np.uint8).reshape(-1, 32)
    ur = None if frame.get("uright") is None else np.ascontiguousarray(frame["uright"], np.float32)
    occ = None if frame.get("occupied") is None else np.ascontiguousarray(frame["occupied"], np.uint8)
    q = np.ascontiguousarray(queries, PROJ_QUERY_DTYPE)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    F = ProjFrame(len(keys), _p(keys), _p(desc), _p(ur), _p(occ), frame["min_x"], frame["min_y"],
                  frame["grid_w_inv"], frame["grid_h_inv"])
    m = np.full(max(len(keys), 1), -1, np.int32)
    nm = ctypes.c_int(0)
    _check(_lib.orbm_search_by_projection(mode, ctypes.byref(F), _p(q), _p(qd), len(q),
                                          float(nnratio), int(th_dist), 1 if check_ori else 0,
                                          device, _p(m), ctypes.byref(nm)),
           "orbm_search_by_projection")
    return m[:len(keys)].copy(), nm.value


class ProjPlan:
    """Batched SearchByProjection (orbm_proj_plan_*): many (frame, queries)
    problems on device-resident data in one set of launches."""

    def __init__(self, max_problems, max_n, max_nq, device=0):
        h = ctypes.c_void_p()
        _check(_lib.orbm_proj_plan_create(max_problems, max_n, max_nq, device, ctypes.byref(h)),
               "orbm_proj_plan_create")
        self._h, self.device = h, device

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbm_proj_plan_destroy(self._h)
            self._h = None

    def search(self, mode, problems, nnratio=0.6, th_dist=100, check_ori=True, stream=None):
        """problems: list of dicts of cuda tensors -- keys [n, 28] u8 (orbx_keypoint
        rows), desc [n, 32] u8, uright [n] f32 or None, occupied [n] u8 or None,
        q [nq] rows of PROJ_QUERY_DTYPE as u8 [nq, 28], qdesc [nq, 32] u8,
        match [n] i32 and nmatches [1] i32 (outputs) -- plus the grid floats
        min_x, min_y, grid_w_inv, grid_h_inv.  Asynchronous."""
        arr = (ProjProblem * max(len(problems), 1))()
        for i, pb in enumerate(problems):
            arr[i].frame = _proj_frame(pb)
            arr[i].q, arr[i].qdesc, arr[i].nq = _dptr(pb["q"]), _dptr(pb["qdesc"]), pb["q"].shape[0]
            arr[i].match, arr[i].nmatches = _dptr(pb["match"]), _dptr(pb["nmatches"])
        _check(_lib.orbm_proj_plan_search(self._h, mode, len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                          float(nnratio), int(th_dist), 1 if check_ori else 0,
                                          _stream_handle(stream)), "orbm_proj_plan_search")


    @staticmethod
    def _build_problems(problems, track):
        arr = (ProjBuildProblem * max(len(problems), 1))()
        for i, pb in enumerate(problems):
            a = arr[i]
            a.camera = proj_camera(pb["camera"])
            pts = pb["points"]
            a.points = ProjPoints(*[_dptr(pts.get(n)) for n in POINT_FIELDS])
            a.npts = pts["pos"].shape[0]
            for n in ("q", "level", "view_cos", "n_in_view", "n_nonfinite"):
                setattr(a, n, _dptr(pb.get(n)))
            if track:
                a.frame = _proj_frame(pb["frame"])
                a.qdesc, a.match, a.nmatches = _dptr(pb["qdesc"]), _dptr(pb["match"]), _dptr(pb["nmatches"])
        return arr

    def project(self, mode, problems, th=1.0, viewing_cos_limit=0.5, level_rule=LEVEL_RULE_NEITHER, stream=None):
        """orbm_proj_plan_project: query rows from map points and a pose, on the
        device.  problems: list of dicts -- camera (a proj_camera dict: host
        values), points (dict of cuda tensors: pos [npts, 3] f32 and, as the
        mode reads them, normal [npts, 3], min_dist_inv, max_dist_inv, max_dist
        f32, octave i32, angle f32, skip u8 or absent), outputs q [npts, 28] u8
        (PROJ_QUERY_DTYPE rows), level [npts] i32, and optionally view_cos
        [npts] f32, n_in_view [1] i32, n_nonfinite [1] i32.  Asynchronous."""
        arr = self._build_problems(problems, False)
        prm = ProjParams(float(th), float(viewing_cos_limit), int(level_rule))
        _check(_lib.orbm_proj_plan_project(self._h, mode, len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                           ctypes.byref(prm), _stream_handle(stream)), "orbm_proj_plan_project")

    def track(self, mode, problems, th=1.0, viewing_cos_limit=0.5, level_rule=LEVEL_RULE_NEITHER, nnratio=0.6,
              th_dist=100, check_ori=True, stream=None):
        """orbm_proj_plan_track: project() followed by search() on the same
        stream.  Each problem adds frame (dict as in search(): keys, desc,
        uright, occupied, grid floats), qdesc [npts, 32] u8 (the map points'
        descriptors) and the outputs match [n] i32 (map-point indices) and
        nmatches [1] i32; q and level may be left out."""
        arr = self._build_problems(problems, True)
        prm = ProjParams(float(th), float(viewing_cos_limit), int(level_rule))
        _check(_lib.orbm_proj_plan_track(self._h, mode, len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                         ctypes.byref(prm), float(nnratio), int(th_dist), 1 if check_ori else 0,
                                         _stream_handle(stream)), "orbm_proj_plan_track")


POINT_FIELDS = ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist", "octave", "angle", "skip")
_POINT_DTYPES = dict(pos=np.float32, normal=np.float32, min_dist_inv=np.float32, max_dist_inv=np.float32,
                     max_dist=np.float32, octave=np.int32, angle=np.float32, skip=np.uint8)


def proj_camera(cam):
    """orbx_proj_camera from a dict: Rcw (3x3), tcw (3), ow (3), fx, fy, cx, cy,
    mbf, min_x, max_x, min_y, max_y, scale_factors (nlevels), log_scale_factor."""
    if isinstance(cam, ProjCamera):
        return cam
    sf = np.asarray(cam["scale_factors"], np.float32).reshape(-1)
    if not 1 <= len(sf) <= PROJ_MAX_LEVELS:
        raise OrbxError(ERR_ARG, "proj_camera: 1 .. %d scale factors expected" % PROJ_MAX_LEVELS)
    c = ProjCamera()
    c.Rcw[:] = np.asarray(cam["Rcw"], np.float32).reshape(9).tolist()
    c.tcw[:] = np.asarray(cam["tcw"], np.float32).reshape(3).tolist()
    c.ow[:] = np.asarray(cam["ow"], np.float32).reshape(3).tolist()
    for n in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y", "log_scale_factor"):
        setattr(c, n, float(np.float32(cam[n])))
    c.nlevels = len(sf)
    c.scale_factors[:len(sf)] = sf.tolist()
    return c


def predict_scale_thresholds(log_scale_factor, nlevels):
    """orbm_predict_scale_thresholds: float32[nlevels - 1], thr[L] = the smallest
    positive ratio whose MapPoint::PredictScale level exceeds L."""
    thr = np.zeros(max(int(nlevels) - 1, 1), np.float32)
    _check(_lib.orbm_predict_scale_thresholds(float(np.float32(log_scale_factor)), int(nlevels), _p(thr)),
           "orbm_predict_scale_thresholds")
    return thr[:max(int(nlevels) - 1, 0)].copy()


def project_points(mode, problems, th=1.0, viewing_cos_limit=0.5, level_rule=LEVEL_RULE_NEITHER, device=0):
    """orbm_project_points on host arrays.  problems: list of (camera dict,
    points dict of numpy arrays named as POINT_FIELDS).  Returns per problem
    (q PROJ_QUERY_DTYPE[npts], level int32[npts], view_cos float32[npts] (mode
    1, else None), n_in_view)."""
    nprob = len(problems)
    cams = (ProjCamera * max(nprob, 1))()
    pts = (ProjPoints * max(nprob, 1))()
    npts = np.zeros(max(nprob, 1), np.int32)
    keep = []
    for i, (cam, P) in enumerate(problems):
        cams[i] = proj_camera(cam)
        arrs = {}
        for n in POINT_FIELDS:
            if P.get(n) is not None:
                arrs[n] = np.ascontiguousarray(P[n], _POINT_DTYPES[n])
        keep.append(arrs)
        pts[i] = ProjPoints(*[_p(arrs.get(n)) for n in POINT_FIELDS])
        npts[i] = len(np.asarray(P["pos"]).reshape(-1, 3))
    total = int(npts[:nprob].sum())
    q = np.zeros(max(total, 1), PROJ_QUERY_DTYPE)
    level = np.zeros(max(total, 1), np.int32)
    vc = np.zeros(max(total, 1), np.float32) if mode == 1 else None
    niv = np.zeros(max(nprob, 1), np.int32)
    prm = ProjParams(float(th), float(viewing_cos_limit), int(level_rule))
    _check(_lib.orbm_project_points(mode, nprob, ctypes.cast(cams, ctypes.c_void_p),
                                    ctypes.cast(pts, ctypes.c_void_p), _p(npts), ctypes.byref(prm), device,
                                    _p(q), _p(level), _p(vc), _p(niv)), "orbm_project_points")
    out, off = [], 0
    for i in range(nprob):
        n = int(npts[i])
        out.append((q[off:off + n].copy(), level[off:off + n].copy(),
                    None if vc is None else vc[off:off + n].copy(), int(niv[i])))
        off += n
    return out


_KF_POINT_DTYPES = dict(pos=np.float32, min_dist_inv=np.float32, max_dist_inv=np.float32, max_dist=np.float32,
                        skip=np.uint8)


def kf_camera(cam):
    """orbx_kf_camera from a dict: Rcw (3x3), tcw (3), fx, fy, cx, cy, min_x,
    max_x, min_y, max_y, scale_factors (nlevels), log_scale_factor, and ow (3;
    the Fuse form) or sR21 (3x3) and t21 (3) (the SearchBySim3 form); what a
    form does not read may be left out."""
    if isinstance(cam, KfCamera):
        return cam
    sf = np.asarray(cam["scale_factors"], np.float32).reshape(-1)
    if not 1 <= len(sf) <= PROJ_MAX_LEVELS:
        raise OrbxError(ERR_ARG, "kf_camera: 1 .. %d scale factors expected" % PROJ_MAX_LEVELS)
    c = KfCamera()
    for n, k in (("Rcw", 9), ("tcw", 3), ("ow", 3), ("sR21", 9), ("t21", 3)):
        if cam.get(n) is not None:
            getattr(c, n)[:] = np.asarray(cam[n], np.float32).reshape(k).tolist()
    for n in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "log_scale_factor"):
        setattr(c, n, float(np.float32(cam[n])))
    c.nlevels = len(sf)
    c.scale_factors[:len(sf)] = sf.tolist()
    return c


def keyframe_project(form, problems, th=3.0, desc_base=None, device=0):
    """orbm_keyframe_project on host arrays: the query rows of ORBmatcher::Fuse
    (KF_FORM_FUSE) or SearchBySim3 (KF_FORM_SIM3) from map points and a pose.
    problems: list of (camera dict, points dict of numpy arrays named as
    KF_POINT_FIELDS); desc_base: None or one int per problem.  Returns per
    problem (q KF_QUERY_DTYPE[npts], level int32[npts], n_live)."""
    nprob = len(problems)
    cams = (KfCamera * max(nprob, 1))()
    pts = (KfPoints * max(nprob, 1))()
    npts = np.zeros(max(nprob, 1), np.int32)
    keep = []
    for i, (cam, P) in enumerate(problems):
        cams[i] = kf_camera(cam)
        arrs = {n: np.ascontiguousarray(P[n], _KF_POINT_DTYPES[n]) for n in KF_POINT_FIELDS if P.get(n) is not None}
        keep.append(arrs)
        pts[i] = KfPoints(*[_p(arrs.get(n)) for n in KF_POINT_FIELDS])
        npts[i] = len(np.asarray(P["pos"]).reshape(-1, 3))
    base = None if desc_base is None else np.ascontiguousarray(desc_base, np.int32).reshape(-1)
    if base is not None and len(base) != nprob:
        raise OrbxError(ERR_ARG, "one desc_base per problem expected")
    total = int(npts[:nprob].sum())
    q = np.zeros(max(total, 1), KF_QUERY_DTYPE)
    level = np.zeros(max(total, 1), np.int32)
    nlive = np.zeros(max(nprob, 1), np.int32)
    _check(_lib.orbm_keyframe_project(int(form), nprob, ctypes.cast(cams, ctypes.c_void_p),
                                      ctypes.cast(pts, ctypes.c_void_p), _p(npts), _p(base), float(th), device,
                                      _p(q), _p(level), _p(nlive)), "orbm_keyframe_project")
    out, off = [], 0
    for i in range(nprob):
        n = int(npts[i])
        out.append((q[off:off + n].copy(), level[off:off + n].copy(), int(nlive[i])))
        off += n
    return out


class KeyframePlan:
    """orbm_kf_plan: the projection of ORBmatcher::Fuse / SearchBySim3 and the
    keyframe window search on device-resident data, asynchronous.  A problem
    is a dict of cuda tensors and host values:
      camera   a kf_camera dict (host values)             [project]
      points   dict: pos [npts, 3] f32, min_dist_inv, max_dist_inv, max_dist
               [npts] f32, skip [npts] u8 or absent        [project]
      npts     the point / query count (taken from points["pos"] or q if absent)
      qdesc    [npts, 32] u8                               [search]
      frame    dict: keys [n, 28] u8 (orbx_keypoint rows), desc [n, 32] u8, and
               the floats min_x, min_y, grid_w_inv, grid_h_inv   [search]
      q        [npts, 20] u8 (KF_QUERY_DTYPE rows): input of search(), output
               of project(), optional output of project_search()
      level    [npts] i32: output of project(), optional for project_search()
      n_live, n_nonfinite   [1] i32, optional outputs      [project]
      best_idx, best_dist   [npts] i32 outputs             [search]
    Point arrays and qdesc of different problems may be the same tensors."""

    def __init__(self, max_problems, max_n, max_queries, device=0):
        h = ctypes.c_void_p()
        _check(_lib.orbm_kf_plan_create(max_problems, max_n, max_queries, device, ctypes.byref(h)),
               "orbm_kf_plan_create")
        self._h, self.device = h, device

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbm_kf_plan_destroy(self._h)
            self._h = None

    @staticmethod
    def _problems(problems, project, search):
        arr = (KfProblem * max(len(problems), 1))()
        for i, pb in enumerate(problems):
            a = arr[i]
            pts = pb.get("points") or {}
            if "npts" in pb:
                a.npts = int(pb["npts"])
            elif project:
                a.npts = pts["pos"].shape[0]
            else:
                a.npts = pb["q"].shape[0]
            if project:
                a.camera = kf_camera(pb["camera"])
                a.points = KfPoints(*[_dptr(pts.get(n)) for n in KF_POINT_FIELDS])
            if search:
                fr = pb["frame"]
                a.frame = KfFrame(fr["keys"].shape[0], _dptr(fr["keys"]), _dptr(fr["desc"]), fr["min_x"],
                                  fr["min_y"], fr["grid_w_inv"], fr["grid_h_inv"])
            for n in ("qdesc", "q", "level", "n_live", "n_nonfinite", "best_idx", "best_dist"):
                setattr(a, n, _dptr(pb.get(n)))
        return arr

    def search(self, problems, stream=None):
        """orbm_kf_plan_search: orbm_keyframe_search's search over the rows in q."""
        arr = self._problems(problems, False, True)
        _check(_lib.orbm_kf_plan_search(self._h, len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                        _stream_handle(stream)), "orbm_kf_plan_search")

    def project(self, form, problems, th=3.0, stream=None):
        """orbm_kf_plan_project: the query rows only."""
        arr = self._problems(problems, True, False)
        _check(_lib.orbm_kf_plan_project(self._h, int(form), len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                         float(th), _stream_handle(stream)), "orbm_kf_plan_project")

    def project_search(self, form, problems, th=3.0, stream=None):
        """orbm_kf_plan_project_search: project() then search() on one stream."""
        arr = self._problems(problems, True, True)
        _check(_lib.orbm_kf_plan_project_search(self._h, int(form), len(problems),
                                                ctypes.cast(arr, ctypes.c_void_p), float(th),
                                                _stream_handle(stream)), "orbm_kf_plan_project_search")


def pose_camera(cam):
    """orbx_pose_camera from a dict: Tcw (3x4 or 4x4, rows 0..2 used), fx, fy,
    cx, cy, mbf, inv_level_sigma2 (nlevels)."""
    if isinstance(cam, PoseCamera):
        return cam
    sg = np.asarray(cam["inv_level_sigma2"], np.float32).reshape(-1)
    if not 1 <= len(sg) <= PROJ_MAX_LEVELS:
        raise OrbxError(ERR_ARG, "pose_camera: 1 .. %d levels expected" % PROJ_MAX_LEVELS)
    c = PoseCamera()
    c.Tcw[:] = np.asarray(cam["Tcw"], np.float32).reshape(-1, 4)[:3].reshape(12).tolist()
    for n in ("fx", "fy", "cx", "cy", "mbf"):
        setattr(c, n, float(np.float32(cam[n])))
    c.nlevels = len(sg)
    c.inv_level_sigma2[:len(sg)] = sg.tolist()
    return c


def pose_optimization(problems, device=0):
    """orbm_pose_optimization (Optimizer::PoseOptimization, batched) on host
    arrays.  problems: list of (camera dict as pose_camera takes, obs dict):
    keys KEYPOINT_DTYPE[n], pos float32[npos, 3], and optionally uright
    float32[n], point_index int32[n] (-1 = no point) or has_point uint8[n].
    Returns per problem (Tcw float32[4, 4], outlier uint8[n], ninliers)."""
    nprob = len(problems)
    cams = (PoseCamera * max(nprob, 1))()
    obs = (PoseObs * max(nprob, 1))()
    keep, ns = [], []
    for i, (cam, O) in enumerate(problems):
        cams[i] = pose_camera(cam)
        keys = np.ascontiguousarray(O["keys"], KEYPOINT_DTYPE).reshape(-1)
        pos = np.ascontiguousarray(O["pos"], np.float32).reshape(-1, 3)
        opt = {k: np.ascontiguousarray(O[k], t).reshape(-1)
               for k, t in (("uright", np.float32), ("point_index", np.int32), ("has_point", np.uint8))
               if O.get(k) is not None}
        for k, a in opt.items():
            if len(a) != len(keys):
                raise OrbxError(ERR_ARG, "pose_optimization: %s has %d entries for %d keys" % (k, len(a), len(keys)))
        keep.append((keys, pos, opt))
        obs[i] = PoseObs(len(keys), _p(keys), _p(opt.get("uright")), _p(pos), _p(opt.get("point_index")),
                         _p(opt.get("has_point")), len(pos))
        ns.append(len(keys))
    total = sum(ns)
    T = np.zeros((max(nprob, 1), 4, 4), np.float32)
    outlier = np.zeros(max(total, 1), np.uint8)
    nin = np.zeros(max(nprob, 1), np.int32)
    _check(_lib.orbm_pose_optimization(nprob, ctypes.cast(cams, ctypes.c_void_p), ctypes.cast(obs, ctypes.c_void_p),
                                       device, _p(T), _p(outlier), _p(nin)), "orbm_pose_optimization")
    out, off = [], 0
    for i, n in enumerate(ns):
        out.append((T[i].copy(), outlier[off:off + n].copy(), int(nin[i])))
        off += n
    return out


class PosePlan:
    """Batched Optimizer::PoseOptimization on device-resident data
    (orbm_pose_plan_*): one launch for all problems, asynchronous."""

    def __init__(self, max_problems, max_n, device=0):
        h = ctypes.c_void_p()
        _check(_lib.orbm_pose_plan_create(max_problems, max_n, device, ctypes.byref(h)), "orbm_pose_plan_create")
        self._h, self.device = h, device

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbm_pose_plan_destroy(self._h)
            self._h = None

    def optimize(self, problems, stream=None):
        """problems: list of dicts -- camera (a pose_camera dict: host values)
        and cuda tensors keys [n, 28] u8 (orbx_keypoint rows), pos [npos, 3]
        f32, optionally uright [n] f32, point_index [n] i32 (-1 = no point; the
        match[] of ProjPlan.track as it stands) or has_point [n] u8, and the
        outputs Tcw_out [16] f32, outlier [n] u8, ninliers [1] i32 and status
        [1] i32 (features dropped for a bad octave or index)."""
        arr = (PoseProblem * max(len(problems), 1))()
        for i, pb in enumerate(problems):
            n = pb["keys"].shape[0]
            _check_dev(pb["keys"], 1, n, "keys", (28,))
            _check_dev(pb["pos"], 4, 0, "pos", (3,))
            for k, sz in (("uright", 4), ("point_index", 4), ("has_point", 1), ("outlier", 1)):
                if pb.get(k) is not None:
                    _check_dev(pb[k], sz, n, k)
            _check_dev(pb["Tcw_out"], 4, 16, "Tcw_out")
            _check_dev(pb["ninliers"], 4, 1, "ninliers")
            _check_dev(pb["status"], 4, 1, "status")
            a = arr[i]
            a.camera = pose_camera(pb["camera"])
            a.obs = PoseObs(n, _dptr(pb["keys"]), _dptr(pb.get("uright")), _dptr(pb["pos"]),
                            _dptr(pb.get("point_index")), _dptr(pb.get("has_point")), pb["pos"].shape[0])
            a.Tcw_out, a.outlier = _dptr(pb["Tcw_out"]), _dptr(pb.get("outlier"))
            a.ninliers, a.status = _dptr(pb["ninliers"]), _dptr(pb["status"])
        _check(_lib.orbm_pose_plan_optimize(self._h, len(problems), ctypes.cast(arr, ctypes.c_void_p),
                                            _stream_handle(stream)), "orbm_pose_plan_optimize")


def compute_distinctive_descriptors(groups, device=0):
    """MapPoint::ComputeDistinctiveDescriptors for a list of (N_m, 32) descriptor
    arrays; returns int32[len(groups)] chosen rows (-1 for empty)."""
    off = np.zeros(len(groups) + 1, np.int32)
    off[1:] = np.cumsum([len(g) for g in groups])
    desc = np.ascontiguousarray(np.concatenate([np.asarray(g, np.uint8).reshape(-1, 32)
                                                for g in groups]) if groups else
                                np.zeros((0, 32), np.uint8))
    best = np.zeros(max(len(groups), 1), np.int32)
    _check(_lib.orbm_compute_distinctive_descriptors(_p(desc), _p(off), len(groups), device,
                                                     _p(best)), "distinctive descriptors")
    return best[:len(groups)].copy()


def undistort_keypoints(kps, K, dist, device=0):
    """Frame::UndistortKeyPoints (cv::undistortPoints, OpenCV 3.4 algorithm)."""
    k = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    K9 = np.ascontiguousarray(K, np.float32).reshape(9)
    D = np.ascontiguousarray(dist, np.float32).reshape(-1)
    out = np.zeros_like(k)
    _check(_lib.orbx_undistort_keypoints(_p(k), len(k), _p(K9), _p(D), len(D), device, _p(out)),
           "orbx_undistort_keypoints")
    return out


# --------------------------------------------------------------------------- batched device path
def _check_dev(t, itemsize, rows, name, tail=None):
    """Validate a caller-supplied cuda tensor before its pointer crosses the C
    ABI: cuda device, contiguous, element size, >= rows leading entries and
    the expected trailing shape (the kernels trust these)."""
    if not getattr(t, "is_cuda", False):
        raise OrbxError(ERR_ARG, "%s: cuda tensor expected" % name)
    if not t.is_contiguous():
        raise OrbxError(ERR_ARG, "%s: contiguous tensor expected" % name)
    if itemsize is not None and t.element_size() != itemsize:
        raise OrbxError(ERR_ARG, "%s: element size %d expected" % (name, itemsize))
    if t.dim() < 1 or t.shape[0] < rows:
        raise OrbxError(ERR_ARG, "%s: at least %d rows expected" % (name, rows))
    if tail is not None and tuple(t.shape[1:]) != tuple(tail):
        raise OrbxError(ERR_ARG, "%s: shape [*, %s] expected, got %s"
                        % (name, ", ".join(map(str, tail)), tuple(t.shape)))


def _stream_handle(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


class Plan:
    """Batched device-resident extraction of `max_batch` frames of W x H."""

    def __init__(self, prm, width, height, max_batch, device=0):
        import torch
        self.params, self.W, self.H, self.max_batch, self.device = prm, width, height, max_batch, device
        h = ctypes.c_void_p()
        _check(_lib.orbx_plan_create(ctypes.byref(prm), width, height, max_batch, device,
                                     ctypes.byref(h)), "orbx_plan_create")
        self._h = h
        self.geo = Geometry()
        _check(_lib.orbx_plan_geometry(self._h, ctypes.byref(self.geo)))
        self.kcap = self.geo.kcap
        dev = torch.device("cuda", device)
        self.kps = torch.empty((max_batch, max(self.kcap, 1), 28), dtype=torch.uint8, device=dev)
        self.desc = torch.empty((max_batch, max(self.kcap, 1), 32), dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(max_batch, dtype=torch.int32, device=dev)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbx_plan_destroy(self._h)
            self._h = None

    def extract(self, frames, stream=None, out=None):
        """frames: cuda uint8 tensor [B, H, W] (row stride W).  Async.
        out: optional (kps [>=B, kcap, 28] u8, desc [>=B, kcap, 32] u8, counts [>=B] i32)."""
        B = frames.shape[0]
        assert frames.dtype.itemsize == 1 and frames.is_contiguous()
        assert frames.shape[1] == self.H and frames.shape[2] == self.W and B <= self.max_batch
        kps, desc, counts = out if out is not None else (self.kps, self.desc, self.counts)
        _check_dev(frames, None, B, "frames")
        _check_dev(kps, 1, B, "kps", (self.kcap, 28))
        _check_dev(desc, 1, B, "desc", (self.kcap, 32))
        _check_dev(counts, 4, B, "counts")
        _check(_lib.orbx_plan_extract(self._h, frames.data_ptr(), B, self.W * self.H, self.W,
                                      kps.data_ptr(), desc.data_ptr(), counts.data_ptr(),
                                      _stream_handle(stream)), "orbx_plan_extract")

    def check(self, stream=None):
        _check(_lib.orbx_plan_check(self._h, _stream_handle(stream)), "orbx_plan_check")

    def debug_counters(self):
        """{'fast_overflow_strips': n, 'fast_dense_strips': m} since the last
        call (synchronises the plan's stream): FAST strips whose corner list
        overflowed, and strips that took the dense post-pass"""
        v, d = ctypes.c_int(0), ctypes.c_int(0)
        _check(_lib.orbx_plan_debug_counters(self._h, ctypes.byref(v)), "orbx_plan_debug_counters")
        _check(_lib.orbx_plan_fast_dense_strips(self._h, ctypes.byref(d)), "orbx_plan_fast_dense_strips")
        return {"fast_overflow_strips": v.value, "fast_dense_strips": d.value}

    def set_options(self, pyramid="auto", brief="auto", fast_post="auto", twins="auto"):
        """pyramid: 'auto' or 'tiles' (k_pyramid, the one pyramid path since
        the round-4 streaming kernels were retired); brief: 'auto' (the
        planner's choice), 'patch' (per-keypoint blur, k_orient_brief) or
        'level' (every level blurred once, k_blur + k_orient_brief_lb).
        fast_post: 'auto' (FAST's post-pass chosen per strip by its corner
        count) or 'dense' (every strip takes the four-wave row-mask form).
        twins: 'auto' (a keypoint kept both in a level and in a level aliasing
        it is computed once and written to both rows) or 'off' (computed once
        per level).  Every combination gives the same results."""
        flags = {"auto": 0, "tiles": ORBX_PLAN_PYR_TILES}[pyramid]
        flags |= {"auto": 0, "patch": ORBX_PLAN_BRIEF_PATCH, "level": ORBX_PLAN_BRIEF_LEVEL}[brief]
        flags |= {"auto": 0, "dense": ORBX_PLAN_FAST_DENSE}[fast_post]
        flags |= {"auto": 0, "off": ORBX_PLAN_NO_TWINS}[twins]
        _check(_lib.orbx_plan_set_options(self._h, flags), "orbx_plan_set_options")

    def level(self, frame, lvl, stream=None):
        """pyramid level `lvl` (>= 1, not aliasing level 0) of frame `frame` of
        the last extract, as a host array (synchronises the stream)"""
        w, h = ctypes.c_int(0), ctypes.c_int(0)
        _check(_lib.orbx_plan_level(self._h, frame, lvl, None, 0, ctypes.byref(w), ctypes.byref(h),
                                    _stream_handle(stream)), "orbx_plan_level")
        out = np.empty((h.value, w.value), np.uint8)
        _check(_lib.orbx_plan_level(self._h, frame, lvl, _p(out), w.value, None, None,
                                    _stream_handle(stream)), "orbx_plan_level")
        return out

    def set_timing(self, enable):
        _check(_lib.orbx_plan_set_timing(self._h, 1 if enable else 0))

    def stage_times(self):
        n = _lib.orbx_stage_count()
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.int32)
        _check(_lib.orbx_plan_stage_times(self._h, _p(ms), _p(cnt), n))
        return {name: (ms[i], int(cnt[i])) for i, name in enumerate(stage_names())}

    def results(self, B):
        """host copies: list of (keypoints structured array, descriptors) for frames 0..B-1"""
        counts = self.counts[:B].cpu().numpy()
        kraw = self.kps[:B].cpu().numpy()
        draw = self.desc[:B].cpu().numpy()
        out = []
        for f in range(B):
            n = int(counts[f])
            k = kraw[f, :n].copy().view(KEYPOINT_DTYPE).reshape(n)
            out.append((k, draw[f, :n].copy()))
        return out


class MatchPlan:
    """Batched brute-force SearchByBoW between extractor frames (single node, top-N).

    zero_tail=True asserts that bytes 24..31 of every descriptor are zero (true
    of Plan.extract outputs) and lets the distance kernels skip them; valu=True
    takes the xor/popcount distance kernel instead of the MFMA one; fold=False
    gives every selected keypoint its own distance row and column instead of
    computing byte-identical descriptors of a list once (same matches)."""

    def __init__(self, max_pairs, kcap, topn=2000, device=0, zero_tail=False, valu=False, fold=True):
        import torch
        h = ctypes.c_void_p()
        _check(_lib.orbm_plan_create(max_pairs, kcap, topn, device, ctypes.byref(h)),
               "orbm_plan_create")
        self._h, self.kcap, self.topn, self.max_pairs = h, kcap, topn, max_pairs
        _check(_lib.orbm_plan_set_options(h, (ORBM_PLAN_ZERO_TAIL if zero_tail else 0)
                                          | (ORBM_PLAN_VALU if valu else 0)
                                          | (0 if fold else ORBM_PLAN_NO_FOLD)), "orbm_plan_set_options")
        dev = torch.device("cuda", device)
        self.match12 = torch.empty((max_pairs, kcap), dtype=torch.int32, device=dev)
        self.nmatches = torch.zeros(max_pairs, dtype=torch.int32, device=dev)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbm_plan_destroy(self._h)
            self._h = None

    def match(self, npairs, kps_a, desc_a, cnt_a, kps_b, desc_b, cnt_b, nnratio=0.6,
              check_ori=True, stream=None, out_offset=0):
        if npairs < 1 or out_offset < 0 or npairs + out_offset > self.max_pairs:
            raise OrbxError(ERR_ARG, "MatchPlan.match: npairs %d + out_offset %d > max_pairs %d"
                            % (npairs, out_offset, self.max_pairs))
        for t, name, shape in ((kps_a, "kps_a", (self.kcap, 28)), (desc_a, "desc_a", (self.kcap, 32)),
                               (kps_b, "kps_b", (self.kcap, 28)), (desc_b, "desc_b", (self.kcap, 32))):
            _check_dev(t, 1, npairs, name, shape)
        _check_dev(cnt_a, 4, npairs, "cnt_a")
        _check_dev(cnt_b, 4, npairs, "cnt_b")
        m = self.match12[out_offset:]
        nm = self.nmatches[out_offset:]
        _check(_lib.orbm_plan_match_frames(self._h, npairs, kps_a.data_ptr(), desc_a.data_ptr(),
                                           cnt_a.data_ptr(), kps_b.data_ptr(), desc_b.data_ptr(),
                                           cnt_b.data_ptr(), float(nnratio), 1 if check_ori else 0,
                                           m.data_ptr(), nm.data_ptr(), _stream_handle(stream)),
               "orbm_plan_match_frames")

    def fold_stats(self):
        """(list1 entries, list1 followers, list2 entries, list2 followers) of the
        last match() call, summed over its pairs; waits for that call."""
        out = np.zeros(4, np.int64)
        _check(_lib.orbm_plan_fold_stats(self._h, _p(out)), "orbm_plan_fold_stats")
        return tuple(int(v) for v in out)

    def set_timing(self, enable):
        _check(_lib.orbm_plan_set_timing(self._h, 1 if enable else 0))

    def stage_times(self):
        n = _lib.orbx_stage_count()
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.int32)
        _check(_lib.orbm_plan_stage_times(self._h, _p(ms), _p(cnt), n))
        return {name: (ms[i], int(cnt[i])) for i, name in enumerate(stage_names())}


class StereoPlan:
    """Batched device stereo matcher (Frame::ComputeStereoMatches) over the
    outputs and pyramids of a left and a right Plan of the same geometry."""

    def __init__(self, plan, max_batch=None, device=0):
        import torch
        max_batch = max_batch or plan.max_batch
        h = ctypes.c_void_p()
        _check(_lib.orbs_plan_create(plan._h, max_batch, ctypes.byref(h)), "orbs_plan_create")
        self._h, self.kcap, self.max_batch = h, plan.kcap, max_batch
        dev = torch.device("cuda", device)
        self.uright = torch.empty((max_batch, max(self.kcap, 1)), dtype=torch.float32, device=dev)
        self.depth = torch.empty((max_batch, max(self.kcap, 1)), dtype=torch.float32, device=dev)
        self.nmatches = torch.zeros(max_batch, dtype=torch.int32, device=dev)

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.orbs_plan_destroy(self._h)
            self._h = None

    def match(self, left, right, frames_l, frames_r, mb, mbf, left_out=None, right_out=None,
              stream=None):
        """frames_*: the cuda [B, H, W] tensors the plans last extracted.  Async."""
        B = frames_l.shape[0]
        if B > self.max_batch or frames_r.shape[0] < B:
            raise OrbxError(ERR_ARG, "StereoPlan.match: batch %d > max_batch %d" % (B, self.max_batch))
        _check_dev(frames_l, 1, B, "frames_l", (left.H, left.W))
        _check_dev(frames_r, 1, B, "frames_r", (left.H, left.W))
        kl, dl, cl = left_out if left_out is not None else (left.kps, left.desc, left.counts)
        kr, dr, cr = right_out if right_out is not None else (right.kps, right.desc, right.counts)
        for t, name, shape in ((kl, "kps_l", (self.kcap, 28)), (dl, "desc_l", (self.kcap, 32)),
                               (kr, "kps_r", (self.kcap, 28)), (dr, "desc_r", (self.kcap, 32))):
            _check_dev(t, 1, B, name, shape)
        _check_dev(cl, 4, B, "counts_l")
        _check_dev(cr, 4, B, "counts_r")
        _check(_lib.orbs_plan_match(self._h, B, left._h, right._h, frames_l.data_ptr(),
                                    frames_r.data_ptr(), left.W * left.H, left.W, kl.data_ptr(),
                                    dl.data_ptr(), cl.data_ptr(), kr.data_ptr(), dr.data_ptr(),
                                    cr.data_ptr(), float(mb), float(mbf), self.uright.data_ptr(),
                                    self.depth.data_ptr(), self.nmatches.data_ptr(),
                                    _stream_handle(stream)), "orbs_plan_match")

    def check(self, stream=None):
        _check(_lib.orbs_plan_check(self._h, _stream_handle(stream)), "orbs_plan_check")

    def set_timing(self, enable):
        _check(_lib.orbs_plan_set_timing(self._h, 1 if enable else 0))

    def stage_times(self):
        n = _lib.orbx_stage_count()
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.int32)
        _check(_lib.orbs_plan_stage_times(self._h, _p(ms), _p(cnt), n))
        return {name: (ms[i], int(cnt[i])) for i, name in enumerate(stage_names())}


def selftest_sincos(x):
    """(sin, cos) the BRIEF kernel uses for each float angle of the cuda float32
    tensor x (radians); returns a cuda float32 tensor [n, 2]."""
    import torch
    out = torch.empty((x.numel(), 2), dtype=torch.float32, device=x.device)
    _check(_lib.orbx_selftest_sincos(x.data_ptr(), x.numel(), out.data_ptr(), None),
           "orbx_selftest_sincos")
    torch.cuda.synchronize(x.device)
    return out


def synth_frames(out, first_idx, kind="rects", stream=None):
    """Fill a cuda uint8 tensor [B, H, W] with synthetic frames (orbx/synth.py spec)."""
    from . import synth
    B, H, W = out.shape
    _check(_lib.orbx_synth_frames(out.data_ptr(), W, H, W * H, B, first_idx, synth.KINDS[kind],
                                  _stream_handle(stream)), "orbx_synth_frames")
