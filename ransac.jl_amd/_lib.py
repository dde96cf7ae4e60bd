"""ctypes binding of libransac_hip.so (include/ransac_hip.h).  Loading fails loudly when the
HIP library has not been built: there is no CPU fallback in the product path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libransac_hip.so")
# the -DRH_DIAG build of the same sources (build.py): the A/B switches of the experiments, RH_* environment variables and
# the rh_dbg_* audits live there and only there.  RH_LIB_VARIANT=diag makes it this process's library (tests marked `diag`,
# tools/fuzz_*.py, the profiling tools); the default is the product library, which reads no environment variable.
SO_PATH_DIAG = os.path.join(_HERE, "libransac_hip_diag.so")
OPTION_UNSET = -(1 << 63)
SCORE_PATH = {"auto": 0, "brute": 1, "groups": 2}
REFIT_PATH = {"auto": 0, "scan": 1, "culled": 2}

PLANE, SPHERE, CYLINDER, CONE = 0, 1, 2, 3
KIND_NAMES = {PLANE: "plane", SPHERE: "sphere", CYLINDER: "cylinder", CONE: "cone"}
SCORE_INT64_WRAP, SCORE_F64 = 0, 1
S_LENGTHC, S_ALLCAND, S_NOFMINSET = 1, 2, 3
RH_OK, RH_E_INVALID, RH_E_NODEVICE, RH_E_NOMEM, RH_E_CAPACITY, RH_E_INTERNAL = 0, -1, -2, -3, -4, -5


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("outwards", C.c_int32), ("v", C.c_double * 10)]


class Params(C.Structure):
    _fields_ = [
        ("eps", C.c_double * 4), ("alpha", C.c_double * 4), ("cos_alpha", C.c_double * 4),
        ("collin_threshold", C.c_double), ("parallelthrdeg", C.c_double), ("cos_parallelthr", C.c_double),
        ("sphere_par", C.c_double), ("minconeopang", C.c_double), ("prob_det", C.c_double),
        ("tau", C.c_int64), ("itermax", C.c_int64),
        ("drawN", C.c_int32), ("minsubsetN", C.c_int32), ("extract_s", C.c_int32), ("terminate_s", C.c_int32),
        ("n_shape_types", C.c_int32), ("shape_types", C.c_int32 * 8),
        ("score_mode", C.c_int32), ("sphere_uses_enabled", C.c_int32), ("sampling_streams", C.c_int32),
        ("octree_sampling", C.c_int32), ("octree_max_depth", C.c_int32),
    ]


class Rng(C.Structure):
    _fields_ = [("s", C.c_uint64 * 4), ("stream", C.POINTER(C.c_uint64)), ("stream_len", C.c_int64),
                ("stream_pos", C.c_int64), ("draws", C.c_int64)]


class Extracted(C.Structure):
    _fields_ = [("shape", Shape), ("n_inpoints", C.c_int64), ("inpoints", C.POINTER(C.c_int64)),
                ("score_E", C.c_double), ("iteration", C.c_int64)]


class Result(C.Structure):
    _fields_ = [("shapes", C.POINTER(Extracted)), ("n_shapes", C.c_int64), ("iterations", C.c_int64),
                ("candidates_scored", C.c_int64), ("scored_left", C.c_int64), ("seconds", C.c_double),
                ("seconds_score", C.c_double), ("seconds_extract", C.c_double), ("seconds_host", C.c_double),
                ("seconds_to_last_extraction", C.c_double), ("arena", C.c_void_p)]


class NormalsParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("orient", C.c_int32), ("radius", C.c_double), ("viewpoint", C.c_double * 3)]


class VoxelParams(C.Structure):
    """rh_voxel_params (include/ransac_hip.h)"""
    _fields_ = [("beta", C.c_double), ("mode", C.c_int32), ("flags", C.c_int32)]


class OutlierParams(C.Structure):
    """rh_outlier_params (include/ransac_hip.h)"""
    _fields_ = [("k", C.c_int32), ("mode", C.c_int32), ("std_mul", C.c_double), ("radius", C.c_double),
                ("threshold", C.c_double)]


class OutlierStats(C.Structure):
    """rh_outlier_stats (include/ransac_hip.h)"""
    _fields_ = [("n_valid", C.c_int64), ("n_kept", C.c_int64), ("mu", C.c_double), ("sigma", C.c_double),
                ("tau", C.c_double), ("nn_median", C.c_double)]


class ClusterParams(C.Structure):
    """rh_cluster_params (include/ransac_hip.h)"""
    _fields_ = [("eps", C.c_double), ("min_pts", C.c_int32), ("min_size", C.c_int32), ("order", C.c_int32),
                ("reserved", C.c_int32)]


class ClusterStats(C.Structure):
    """rh_cluster_stats (include/ransac_hip.h)"""
    _fields_ = [("n_clusters", C.c_int64), ("n_core", C.c_int64), ("n_border", C.c_int64), ("n_noise", C.c_int64),
                ("n_small", C.c_int64), ("largest", C.c_int64)]


class SegmentParams(C.Structure):
    """rh_segment_params (include/ransac_hip.h)"""
    _fields_ = [("k", C.c_int32), ("flags", C.c_int32), ("radius", C.c_double), ("cos_angle", C.c_double),
                ("curv_max", C.c_double), ("dist_max", C.c_double), ("min_size", C.c_int32), ("order", C.c_int32)]


class SegmentStats(C.Structure):
    """rh_segment_stats (include/ransac_hip.h)"""
    _fields_ = [("n_regions", C.c_int64), ("n_seed", C.c_int64), ("n_border", C.c_int64), ("n_unassigned", C.c_int64),
                ("n_invalid", C.c_int64), ("n_small", C.c_int64), ("largest", C.c_int64)]


class OrientParams(C.Structure):
    """rh_orient_params (include/ransac_hip.h)"""
    _fields_ = [("k", C.c_int32), ("anchor", C.c_int32), ("radius", C.c_double), ("up", C.c_double * 3)]


class OrientStats(C.Structure):
    """rh_orient_stats (include/ransac_hip.h)"""
    _fields_ = [("n_vertices", C.c_int64), ("n_edges", C.c_int64), ("n_components", C.c_int64), ("n_tree_edges", C.c_int64),
                ("n_flipped", C.c_int64), ("n_inconsistent", C.c_int64), ("largest_component", C.c_int64),
                ("min_tree_absdot", C.c_double)]


class DistanceParams(C.Structure):
    """rh_distance_params (include/ransac_hip.h)"""
    _fields_ = [("radius", C.c_double), ("threshold", C.c_double), ("metric", C.c_int32), ("reserved", C.c_int32)]


class DistanceStats(C.Structure):
    """rh_distance_stats (include/ransac_hip.h)"""
    _fields_ = [("n_valid", C.c_int64), ("n_within", C.c_int64), ("argmax", C.c_int64), ("mean", C.c_double),
                ("rms", C.c_double), ("max", C.c_double), ("median", C.c_double)]


class RegisterParams(C.Structure):
    """rh_register_params (include/ransac_hip.h)"""
    _fields_ = [("radius", C.c_double), ("rot_tol", C.c_double), ("trans_tol", C.c_double), ("metric", C.c_int32),
                ("max_iter", C.c_int32)]


class RegisterResult(C.Structure):
    """rh_register_result (include/ransac_hip.h)"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_valid", C.c_int64), ("rms", C.c_double)]


class GlobalParams(C.Structure):
    """rh_global_params (include/ransac_hip.h)"""
    _fields_ = [("trials", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("tau", C.c_double),
                ("edge_ratio", C.c_double), ("min_edge", C.c_double)]


class GlobalResult(C.Structure):
    """rh_global_result (include/ransac_hip.h)"""
    _fields_ = [("status", C.c_int32), ("best_trial", C.c_int32), ("best_count", C.c_int32), ("n_valid_trials", C.c_int32)]


KNN_MAX_K = 63
DESC_DIM, DESC_MAX = 33, 7938
MATCH_MUTUAL = 1
GLOBAL_MAX_TRIALS = 1 << 20
GLOB_OK, GLOB_NO_TRIAL = 0, 1
GLOB_STATUS_NAMES = {GLOB_OK: "ok", GLOB_NO_TRIAL: "no_trial"}
DIST_POINT, DIST_PLANE = 0, 1
REG_CONVERGED, REG_MAX_ITER, REG_DEGENERATE, REG_TOO_FEW = 0, 1, 2, 3
REG_STATUS_NAMES = {REG_CONVERGED: "converged", REG_MAX_ITER: "max_iter", REG_DEGENERATE: "degenerate", REG_TOO_FEW: "too_few"}
REG_MAX_ITERATIONS = 1000
OUT_BLOCK_POINTS = 1024
OUT_STATISTICAL, OUT_ABSOLUTE, OUT_RADIUS = 0, 1, 2
CLUSTER_BY_INDEX, CLUSTER_BY_SIZE = 0, 1
PT_NOISE, PT_BORDER, PT_CORE = 0, 1, 2
SEG_UNSIGNED = 1
ORI_ANCHOR_FIRST, ORI_ANCHOR_TOP = 0, 1
VOX_FIRST, VOX_CENTROID = 0, 1
VOX_ALIGN_NORMALS = 1
EXT_EMPTY, EXT_NO_DIRECTION, EXT_INVALID = 1, 2, 4
ASSIGN_NO_NORMALS, ASSIGN_ENABLED_ONLY = 1, 2
ASSIGN_MAX_SHAPES = 1024


class Extent(C.Structure):
    """rh_extent: the frame, box and residuals of a shape's points (include/ransac_hip.h)"""
    _fields_ = [("n", C.c_int64), ("kind", C.c_int32), ("flags", C.c_int32), ("origin", C.c_double * 3),
                ("frame", C.c_double * 9), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("centroid", C.c_double * 3),
                ("lam", C.c_double * 3), ("dist_rms", C.c_double), ("dist_maxabs", C.c_double)]


class RansacHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libransac_hip error %d: %s" % (code, msg))
        self.code = code


_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_sp, _pp, _vp = C.POINTER(Shape), C.POINTER(Params), C.c_void_p

# every symbol include/ransac_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "rh_version": (C.c_int, []),
    "rh_last_error": (C.c_char_p, []),
    "rh_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "rh_default_params": (None, [_pp]),
    "rh_params_finalize": (None, [_pp]),
    "rh_shape_finalize": (None, [_sp]),
    "rh_cloud_create": (C.c_int, [_dp, _dp, C.c_int64, _i64p, C.c_int64, C.c_int, C.POINTER(_vp)]),
    "rh_cloud_destroy": (C.c_int, [_vp]),
    "rh_cloud_info": (C.c_int, [_vp, _i64p, _i64p, C.POINTER(C.c_int)]),
    "rh_cloud_set_enabled": (C.c_int, [_vp, _u64p, C.c_int64]),
    "rh_cloud_get_enabled": (C.c_int, [_vp, _u64p, C.c_int64]),
    "rh_cloud_enable_all": (C.c_int, [_vp]),
    "rh_cloud_count_enabled": (C.c_int, [_vp, _i64p]),
    "rh_score_batch": (C.c_int, [_vp, _sp, C.c_int32, _pp, _i32p, _u64p]),
    "rh_score_batch_dev": (C.c_int, [_vp, _vp, C.c_int32, _pp, _vp, _vp]),
    "rh_cloud_set_stream": (C.c_int, [_vp, _vp, C.c_int]),
    "rh_score_batch_dev_timed": (C.c_int, [_vp, _vp, C.c_int32, _pp, _vp, _vp, C.POINTER(C.c_float)]),
    "rh_refit": (C.c_int, [_vp, _sp, _pp, _i64p, C.c_int64, _i64p]),
    "rh_refit_component": (C.c_int, [_vp, _sp, _pp, C.c_double, C.c_int32, _i64p, C.c_int64, _i64p, _i64p, _i32p]),
    "rh_cloud_set_component_filter": (C.c_int, [_vp, C.c_double, C.c_int32]),
    "rh_cloud_get_component_filter": (C.c_int, [_vp, _dp, _i32p]),
    "rh_refit_lsq": (C.c_int, [_vp, _sp, _pp, C.c_int32, _sp, _i64p, _dp, _i32p]),
    "rh_invalidate": (C.c_int, [_vp, _i64p, C.c_int64]),
    "rh_select_enabled": (C.c_int, [_vp, _i64p, C.c_int32, _i64p]),
    "rh_sample_sets": (C.c_int, [_vp, C.c_int32, C.POINTER(Rng), C.c_int32, _i64p, _i32p, _i32p]),
    "rh_fit_sets": (C.c_int, [_dp, _dp, _i64p, _i32p, C.c_int32, C.c_int32, _pp, C.c_int32, _sp, _i32p, C.c_int32, _i32p]),
    "rh_fit": (C.c_int, [C.c_int, _dp, _dp, C.c_int32, _pp, _sp, _i32p]),
    "rh_fit_f32": (C.c_int, [C.c_int, _dp, _dp, C.c_int32, _pp, _sp, _i32p]),
    "rh_estimatescore": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, _dp, _dp, _dp]),
    "rh_prob": (C.c_double, [C.c_double, C.c_int64, C.c_int64, C.c_int64]),
    "rh_rng_seed": (None, [C.POINTER(Rng), C.c_uint64]),
    "rh_rng_range": (C.c_int64, [C.POINTER(Rng), C.c_int64]),
    "rh_ransac": (C.c_int, [_vp, _dp, _dp, _pp, C.POINTER(Rng), C.POINTER(Result)]),
    "rh_ransac_f32": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _pp, C.POINTER(Rng), C.POINTER(Result)]),
    "rh_result_free": (None, [C.POINTER(Result)]),
    "rh_largestconncomp": (C.c_int, [_u8p, C.c_int32, C.c_int32, C.c_int32, C.c_int, _i64p, C.c_int64, _i64p]),
    "rh_bitmapparameters": (C.c_int, [_dp, _u8p, _i64p, C.c_int64, C.c_double, _i32p, _i32p, _dp, _dp, _u8p, _i64p]),
    "rh_last_refit_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rh_timer_start": (C.c_int, [_vp]),
    "rh_timer_stop": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "rh_cloud_sync": (C.c_int, [_vp]),
    "rh_dev_alloc": (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    "rh_cloud_create_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.c_int, C.POINTER(_vp)]),
    "rh_shape_finalize_f32": (None, [C.POINTER(Shape)]),
    "rh_mp_open": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(_vp)]),
    "rh_mp_close": (C.c_int, [_vp]),
    "rh_mp_allgather": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "rh_ransac_mp": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Params), C.POINTER(Rng), _vp, C.POINTER(Result)]),
    "rh_dev_free": (C.c_int, [_vp, _vp]),
    "rh_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "rh_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    "rh_octree_build": (C.c_int, [_dp, C.c_int64, C.POINTER(C.c_void_p)]),
    "rh_octree_build_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_void_p)]),
    "rh_octree_destroy": (C.c_int, [_vp]),
    "rh_octree_info": (C.c_int, [_vp, _i32p, _i32p, _i32p]),
    "rh_octree_findleaf": (C.c_int, [_vp, _dp, _i32p]),
    "rh_octree_getnthcell": (C.c_int, [_vp, C.c_int32, C.c_int32, _i32p]),
    "rh_octree_node_info": (C.c_int, [_vp, C.c_int32, _dp, _dp, _i32p, _i32p, _i32p, C.POINTER(C.c_int64)]),
    "rh_octree_node_points": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64), C.c_int64]),
    "rh_octree_cell_enabled": (C.c_int, [_vp, _vp, C.c_int32, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]),
    "rh_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "rh_get_option": (C.c_int, [_vp, C.c_char_p, _i64p, _i32p]),
    "rh_score_launch_info": (C.c_int, [_vp, C.POINTER(C.c_int32)]),
    "rh_last_list_launch_ms": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    "rh_build_variant": (C.c_int, []),
    "rh_cloud_create_ms": (C.c_int, [_vp, _dp]),
    "rh_comm_unique_id": (C.c_int, [_vp]),
    "rh_comm_create": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.POINTER(_vp)]),
    "rh_comm_destroy": (C.c_int, [_vp]),
    "rh_score_batch_allreduce_dev": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _pp, _vp]),
    "rh_comm_fence": (C.c_int, [_vp, _vp]),
    "rh_comm_sync": (C.c_int, [_vp]),
    "rh_shape_extents": (C.c_int, [_vp, _sp, C.c_int32, _i64p, _i64p, C.POINTER(Extent)]),
    "rh_shape_extents_dev": (C.c_int, [_vp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp]),
    "rh_result_extents": (C.c_int, [_vp, C.POINTER(Result), C.POINTER(Extent)]),
    "rh_assign_points": (C.c_int, [_dp, _dp, C.c_int64, _sp, C.c_int32, _pp, C.c_int32, C.c_int, _i32p, _dp, _i64p, _i64p, _i64p]),
    "rh_assign_points_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, _sp, C.c_int32, _pp, C.c_int32, C.c_int,
                                       _i32p, _dp, _i64p, _i64p, _i64p]),
    "rh_cloud_assign": (C.c_int, [_vp, _sp, C.c_int32, _pp, C.c_int32, _i32p, _dp, _i64p, _i64p, _i64p]),
    "rh_cloud_assign_dev": (C.c_int, [_vp, _vp, C.c_int32, _pp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "rh_estimate_normals": (C.c_int, [_dp, C.c_int64, C.POINTER(NormalsParams), _dp, C.c_int, _dp, _dp, _i32p]),
    "rh_estimate_normals_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(NormalsParams), C.POINTER(C.c_float),
                                          C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32p]),
    "rh_cluster": (C.c_int, [_dp, C.c_int64, C.POINTER(ClusterParams), C.c_int, _i32p, _u8p, C.c_int64, _i64p, _i64p, _i64p, _i64p,
                             C.POINTER(ClusterStats)]),
    "rh_cluster_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(ClusterParams), C.c_int, _i32p, _u8p, C.c_int64, _i64p,
                                 _i64p, _i64p, _i64p, C.POINTER(ClusterStats)]),
    "rh_segment_smooth": (C.c_int, [_dp, _dp, _dp, C.c_int64, C.POINTER(SegmentParams), C.c_int, _i32p, _u8p, C.c_int64, _i64p, _i64p,
                                    _i64p, _i64p, C.POINTER(SegmentStats)]),
    "rh_segment_smooth_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64,
                                        C.POINTER(SegmentParams), C.c_int, _i32p, _u8p, C.c_int64, _i64p, _i64p, _i64p, _i64p,
                                        C.POINTER(SegmentStats)]),
    "rh_orient_normals": (C.c_int, [_dp, _dp, C.c_int64, C.POINTER(OrientParams), C.c_int, _dp, _i32p, _i32p, C.POINTER(OrientStats)]),
    "rh_orient_normals_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(OrientParams), C.c_int,
                                        C.POINTER(C.c_float), _i32p, _i32p, C.POINTER(OrientStats)]),
    "rh_voxel_downsample": (C.c_int, [_dp, _dp, C.c_int64, C.POINTER(VoxelParams), C.c_int, _dp, _dp, _i64p, _i32p, C.c_int64,
                                      _i32p, _i64p, _i64p]),
    "rh_voxel_downsample_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(VoxelParams), C.c_int,
                                          C.POINTER(C.c_float), C.POINTER(C.c_float), _i64p, _i32p, C.c_int64, _i32p, _i64p, _i64p]),
    "rh_knn": (C.c_int, [_dp, C.c_int64, C.c_int32, C.c_double, C.c_int, _i32p, _dp, _i32p]),
    "rh_knn_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.c_int32, C.c_double, C.c_int, _i32p, _dp, _i32p]),
    "rh_knn_query": (C.c_int, [_dp, C.c_int64, _dp, C.c_int64, C.c_int32, C.c_double, C.c_int, _i32p, _dp, _i32p]),
    "rh_knn_query_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float), C.c_int64, C.c_int32, C.c_double, C.c_int,
                                   _i32p, _dp, _i32p]),
    "rh_cloud_distance": (C.c_int, [_dp, _dp, C.c_int64, _dp, C.c_int64, C.POINTER(DistanceParams), C.c_int, _dp, _i32p,
                                    C.POINTER(DistanceStats)]),
    "rh_cloud_distance_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float), C.c_int64,
                                        C.POINTER(DistanceParams), C.c_int, _dp, _i32p, C.POINTER(DistanceStats)]),
    "rh_register": (C.c_int, [_dp, _dp, C.c_int64, _dp, C.c_int64, C.POINTER(RegisterParams), _dp, C.c_int, _dp,
                              C.POINTER(RegisterResult), _i32p, _dp]),
    "rh_register_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float), C.c_int64,
                                  C.POINTER(RegisterParams), _dp, C.c_int, _dp, C.POINTER(RegisterResult), _i32p, _dp]),
    "rh_describe": (C.c_int, [_dp, _dp, C.c_int64, C.c_int32, C.c_double, C.c_int, _u16p, _i32p]),
    "rh_describe_f32": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int64, C.c_int32, C.c_double, C.c_int, _u16p,
                                  _i32p]),
    "rh_match_features": (C.c_int, [_u16p, C.c_int64, _u16p, C.c_int64, C.c_int32, C.c_int, _i32p, _u32p]),
    "rh_register_global": (C.c_int, [_dp, C.c_int64, _dp, C.c_int64, _i32p, _i32p, C.c_int64, C.POINTER(GlobalParams), _i32p,
                                     C.c_int, _dp, C.POINTER(GlobalResult), _i32p]),
    "rh_register_global_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float), C.c_int64, _i32p, _i32p, C.c_int64,
                                         C.POINTER(GlobalParams), _i32p, C.c_int, _dp, C.POINTER(GlobalResult), _i32p]),
    "rh_remove_outliers": (C.c_int, [_dp, C.c_int64, C.POINTER(OutlierParams), C.c_int, _u8p, _i32p, C.c_int64, _i64p, _dp,
                                     C.POINTER(OutlierStats)]),
    "rh_remove_outliers_f32": (C.c_int, [C.POINTER(C.c_float), C.c_int64, C.POINTER(OutlierParams), C.c_int, _u8p, _i32p,
                                         C.c_int64, _i64p, _dp, C.POINTER(OutlierStats)]),
}

class DbgCand(C.Structure):
    """rh_dbg_cand (include/ransac_hip_diag.h)"""
    _fields_ = [("slot", C.c_int64), ("level", C.c_int32), ("pad", C.c_int32), ("shape", Shape)]


# include/ransac_hip_diag.h: exported by the diag build only
DIAG_SIGNATURES = {
    "rh_dbg_sample_fit": (C.c_int, [_vp, _pp, C.c_uint64, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_int32, C.POINTER(DbgCand),
                                    C.c_int32, _i32p, _u64p, _i32p, _i32p]),
    "rh_dbg_cls_audit": (C.c_int, [_vp, _sp, C.c_int32, _pp, _dp]),
    "rh_dbg_cls_soundness": (C.c_int, [_vp, _sp, C.c_int32, _pp, C.POINTER(C.c_uint64)]),
    "rh_dbg_cls_soundness_tiles": (C.c_int, [_vp, _sp, C.c_int32, _pp, C.POINTER(C.c_uint64)]),
    "rh_dbg_cls_soundness_nsig": (C.c_int, [_vp, _sp, C.c_int32, _pp, C.POINTER(C.c_uint64)]),
    "rh_dbg_nsig": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_uint32), _dp, C.c_int64, _i32p]),
    "rh_dbg_group_boxes": (C.c_int, [_vp, _dp, C.c_int64, C.POINTER(C.c_int64)]),
    "rh_dbg_kd_shape": (C.c_int, [C.c_int64, C.c_int, _i64p, _i64p, C.c_int64, _i64p, C.c_int64, _i64p, C.c_int64]),
    "rh_dbg_plane_order": (C.c_int, [_vp, _i64p, _dp, _dp, _i32p, C.POINTER(C.c_float), C.POINTER(C.c_uint32), _u64p]),
    "rh_dbg_cylbox": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_int, _dp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    "rh_dbg_cls_round": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_int, C.c_int64, _dp, _dp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                   C.POINTER(C.c_float), _dp]),
    "rh_dbg_books2": (C.c_int, [C.POINTER(C.c_float), C.c_int64, _i32p, _u64p, _u64p, _u8p]),
    "rh_dbg_books2_inplace": (C.c_int, [C.POINTER(C.c_float), C.c_int64, _u64p, _i32p, _u64p, _u64p]),
    "rh_dbg_cls_u2": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_int, C.c_int64, _dp, _dp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.POINTER(C.c_float)]),
    "rh_dbg_conebox": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_int, _dp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_float)]),
    "rh_dbg_cls_cone": (C.c_int, [_sp, _pp, C.c_double, C.c_double, C.c_int, C.c_int64, _dp, _dp, C.c_int, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_float), _dp]),
    "rh_dbg_oct_search_selftest": (C.c_int, [C.c_int64, C.c_uint64, C.c_int64, C.POINTER(C.c_int64)]),
    "rh_dbg_enabled_events": (C.c_int, [_u8p, C.c_int64, C.c_int32, C.POINTER(C.c_uint16)]),
    "rh_dbg_s4_stats": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    "rh_dbg_wave_keys": (C.c_int, [C.POINTER(C.c_uint32), _u8p, _i32p, C.c_int32, C.c_int32, C.c_int, C.c_int, _i32p, _i32p, _i32p]),
}

_libs = {}


def variant():
    """which build this process uses by default: "product" (libransac_hip.so) unless RH_LIB_VARIANT=diag"""
    v = os.environ.get("RH_LIB_VARIANT", "product")
    if v not in ("product", "diag"):
        raise RuntimeError("RH_LIB_VARIANT=%r: expected 'product' or 'diag'" % v)
    return v


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (SONAME
    libamdhip64.so.7, the name libransac_hip.so needs) and loads it by file name: if the system copy
    under /opt/rocm is mapped first, a later `import torch` maps a SECOND runtime that finds no device
    ("no ROCm-capable device is detected").  When torch is installed but not imported yet, map its copy
    first so both sides bind to the same one (RH_SYSTEM_HIP=1 skips this)."""
    import sys
    if "torch" in sys.modules or os.environ.get("RH_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (ImportError, OSError, ValueError):
        pass


def lib(which=None):
    """The loaded library (which = None: this process's default variant, see variant()).  Raises if the shared object is
    missing (run `python -c 'import __graft_entry__ as g; g.build()'` or `python ransac.jl_amd/build.py`)."""
    which = which or variant()
    L = _libs.get(which)
    if L is None:
        path = SO_PATH if which == "product" else SO_PATH_DIAG
        if os.environ.get("RH_LIB_PATH"):   # kernel A/B runs (tools/): another build of this variant of the library
            path = os.environ["RH_LIB_PATH"]
        if not os.path.exists(path):
            raise RuntimeError(
                "%s is missing: the HIP extension has not been built and this package has no CPU "
                "fallback (build it with ransac.jl_amd/build.py)" % path)
        _share_torch_hip_runtime()
        L = C.CDLL(path)
        sigs = dict(SIGNATURES)
        if which == "diag":
            sigs.update(DIAG_SIGNATURES)
        for name, (res, args) in sigs.items():
            f = getattr(L, name, None)
            if f is None and os.environ.get("RH_LIB_PATH"):   # (an older build in an A/B run: it lacks what was added since)
                continue
            if f is None:
                raise AttributeError("%s does not export %s" % (path, name))
            f.restype = res
            f.argtypes = args
        if L.rh_build_variant() != (1 if which == "diag" else 0):
            raise RuntimeError("%s is not the %s build" % (path, which))
        _libs[which] = L
    return L


def check(rc):
    if rc != RH_OK:
        raise RansacHipError(rc, lib().rh_last_error().decode("utf-8", "replace"))
    return rc
