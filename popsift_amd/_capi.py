"""ctypes binding of the C ABI in include/popsift_hip.h (libpopsift_hip.so).

This is the only way Python reaches the extraction path: there is no CPU
fallback.  If the HIP library is missing or fails to load, importing the
symbols raises -- loudly -- instead of silently computing somewhere else.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# POPSIFT_HIP_LIB: load another build of the SAME library (tools/build_variants.sh experiment builds); never a fallback
LIB_PATH = os.environ.get("POPSIFT_HIP_LIB") or os.path.join(_HERE, "libpopsift_hip.so")

MAX_OCTAVES = 20
ORI_MAX = 4

OK = 0
ERR_INVALID, ERR_DEVICE, ERR_NO_DEVICE, ERR_OOM, ERR_STATE, ERR_TOO_SMALL = -1, -2, -3, -4, -5, -6

SIFT_POPSIFT, SIFT_OPENCV, SIFT_VLFEAT = 0, 1, 2
GAUSS_VLFEAT_COMPUTE, GAUSS_VLFEAT_RELATIVE, GAUSS_VLFEAT_RELATIVE_ALL = 0, 1, 2
GAUSS_OPENCV_COMPUTE, GAUSS_FIXED9, GAUSS_FIXED15 = 3, 4, 5
DESC_LOOP, DESC_ILOOP, DESC_GRID, DESC_IGRID, DESC_NOTILE = 0, 1, 2, 3, 4
NORM_ROOTSIFT, NORM_CLASSIC = 0, 1
SCALE_DEFAULT, SCALE_DIRECT = 0, 1  # params.scale_direct (not Config::ScalingMode's enum values)
ORDER_ARRIVAL, ORDER_RASTER = 0, 1  # params.feature_order: POPSIFT_HIP_ORDER_* (tests/order_rule.py states the raster rule)
ORDER_CHUNK = 1024  # POPSIFT_HIP_ORDER_CHUNK: records per workgroup of the ordering pass
STRONGEST_CHUNK = 1024  # POPSIFT_HIP_STRONGEST_CHUNK: records per workgroup of the keep-strongest pass


class Params(C.Structure):
    """popsift_hip_params"""
    _fields_ = [
        ("octaves", C.c_int32), ("levels", C.c_int32), ("sigma", C.c_float),
        ("edge_limit", C.c_float), ("threshold", C.c_float), ("upscale_factor", C.c_float),
        ("sift_mode", C.c_int32), ("gauss_mode", C.c_int32), ("desc_mode", C.c_int32),
        ("norm_mode", C.c_int32), ("norm_multi", C.c_int32), ("max_extrema", C.c_int32),
        ("assume_initial_blur", C.c_int32), ("initial_blur", C.c_float),
        ("filter_grid_size", C.c_int32), ("filter_max_extrema", C.c_int32), ("filter_sorting", C.c_int32),
        ("store_dog", C.c_int32), ("scale_direct", C.c_int32), ("feature_order", C.c_int32),
    ]


class Report(C.Structure):
    """popsift_hip_report"""
    _fields_ = [
        ("num_octaves", C.c_int32), ("base_w", C.c_int32), ("base_h", C.c_int32),
        ("ext_ct", C.c_int32 * MAX_OCTAVES), ("ori_ct", C.c_int32 * MAX_OCTAVES),
        ("ext_total", C.c_int32), ("ori_total", C.c_int32),
        ("ms_device", C.c_float), ("ms_blur", C.c_float), ("blur_launches", C.c_int32),
        ("blur_alg_bytes", C.c_double), ("pyramid_pixels", C.c_double),
        ("big_alg_bytes", C.c_double), ("ms_big", C.c_float), ("big_launches", C.c_int32),
        ("ms_stage", C.c_float * 8),
    ]


class DeviceInfo(C.Structure):
    """popsift_hip_device_info"""
    _fields_ = [
        ("name", C.c_char * 256), ("arch_major", C.c_int32), ("arch_minor", C.c_int32),
        ("total_mem", C.c_uint64), ("lds_per_block", C.c_uint64), ("wave_size", C.c_int32),
        ("max_threads_per_block", C.c_int32), ("max_threads_per_cu", C.c_int32),
        ("max_block", C.c_int32 * 3), ("max_grid", C.c_int32 * 3), ("cu_count", C.c_int32),
        ("concurrent_kernels", C.c_int32), ("can_map_host", C.c_int32), ("unified_addressing", C.c_int32),
    ]


class MatchOpts(C.Structure):
    """popsift_hip_match_opts"""
    _fields_ = [("ratio", C.c_float), ("max_dist2", C.c_float), ("cross_check", C.c_int32), ("reserved", C.c_int32)]


class GuidedOpts(C.Structure):
    """popsift_hip_guided_opts"""
    _fields_ = [("model", C.c_int32), ("M", C.c_float * 9), ("max_err", C.c_float), ("ratio", C.c_float),
                ("max_dist2", C.c_float), ("cross_check", C.c_int32), ("reserved", C.c_int32 * 2)]


class RansacOpts(C.Structure):
    """popsift_hip_ransac_opts"""
    _fields_ = [("model", C.c_int32), ("hypotheses", C.c_int32), ("max_err", C.c_float), ("seed", C.c_uint32),
                ("reserved", C.c_int32 * 2)]


class EpipolarOpts(C.Structure):
    """popsift_hip_epipolar_opts"""
    _fields_ = [("hypotheses", C.c_int32), ("max_err", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_int32 * 3)]


class RefitOpts(C.Structure):
    """popsift_hip_refit_opts"""
    _fields_ = [("model", C.c_int32), ("rounds", C.c_int32), ("max_err", C.c_float), ("M", C.c_float * 9),
                ("reserved", C.c_int32 * 4)]


class RansacManyOpts(C.Structure):
    """popsift_hip_ransac_many_opts"""
    _fields_ = [("kind", C.c_int32), ("hypotheses", C.c_int32), ("max_err", C.c_float), ("seed", C.c_uint32),
                ("reserved", C.c_int32 * 4)]


FEATURE_DTYPE = np.dtype([
    ("debug_octave", np.int32), ("xpos", np.float32), ("ypos", np.float32),
    ("sigma", np.float32), ("num_ori", np.int32),
    ("orientation", np.float32, (ORI_MAX,)), ("desc_idx", np.int32, (ORI_MAX,)),
])
MATCH_DTYPE = np.dtype([("best", np.int32), ("second", np.int32), ("accept", np.int32),
                        ("dist_best", np.float32), ("dist_second", np.float32)])
# popsift_hip_pair: one correspondence of DevFeatures.match_pairs
PAIR_DTYPE = np.dtype([("l", np.int32), ("r", np.int32), ("dist_best", np.float32), ("dist_second", np.float32)])
# popsift_hip_ransac_result: what Verifier.ransac returns beside the mask
RANSAC_RESULT_DTYPE = np.dtype([("H", np.float32, (9,)), ("n_inliers", np.int32), ("hypothesis", np.int32),
                                ("n_valid", np.int32), ("reserved", np.int32)])
# popsift_hip_refit_result: what Verifier.refit returns beside the mask
REFIT_RESULT_DTYPE = np.dtype([("M", np.float32, (9,)), ("n_inliers", np.int32), ("n_start", np.int32), ("rounds", np.int32),
                               ("stop", np.int32)])
REFIT_HOMOGRAPHY, REFIT_AFFINE, REFIT_EPIPOLAR = 0, 1, 2     # POPSIFT_HIP_REFIT_*: the kind of model of Verifier.refit
REFITS = {"homography": REFIT_HOMOGRAPHY, "affine": REFIT_AFFINE, "epipolar": REFIT_EPIPOLAR}
# POPSIFT_HIP_REFIT_STOP_*: why Verifier.refit stopped
REFIT_STOP_ROUNDS, REFIT_STOP_CONVERGED, REFIT_STOP_NOT_BETTER, REFIT_STOP_NO_FIT, REFIT_STOP_NO_SUPPORT = range(5)
# POPSIFT_HIP_REFIT_*: pairs per workgroup of the accumulating kernel, the most rounds, sums per round of the trace
REFIT_CHUNK, REFIT_MAX_ROUNDS, REFIT_SLOTS = 1024, 16, 45
# POPSIFT_HIP_RANSAC_MANY_*: (list, hypothesis) records of a group of Verifier.ransac_many, pairs of a scoring segment
RANSAC_MANY_GROUP, RANSAC_MANY_SEGMENT = 1 << 20, 256
MODEL_HOMOGRAPHY, MODEL_AFFINE = 0, 1
MODELS = {"homography": MODEL_HOMOGRAPHY, "affine": MODEL_AFFINE}
RANSAC_CHUNK, RANSAC_HYP_BLOCK = 1024, 64  # POPSIFT_HIP_RANSAC_*: pairs / hypotheses per workgroup of the scoring kernel
EPIPOLAR_SAMPLE = 8                        # POPSIFT_HIP_EPIPOLAR_SAMPLE: pairs per hypothesis of Verifier.epipolar
GUIDE_HOMOGRAPHY, GUIDE_EPIPOLAR = 0, 1    # POPSIFT_HIP_GUIDE_*: the model of DevFeatures.match_guided
GUIDES = {"homography": GUIDE_HOMOGRAPHY, "affine": GUIDE_HOMOGRAPHY, "epipolar": GUIDE_EPIPOLAR}
# POPSIFT_HIP_GUIDED_*: left rows per workgroup, right positions per step, queue entries of the guided matcher's kernel
GUIDED_ROWS, GUIDED_STEP, GUIDED_QUEUE = 64, 256, 512
EXTREMUM_DTYPE = np.dtype([
    ("xpos", np.float32), ("ypos", np.float32), ("lpos", np.int32),
    ("sigma", np.float32), ("octave", np.int32), ("cell", np.int32),
])
# popsift_hip_frame: a caller-supplied keypoint for Context.describe (octave / level -1: derived from sigma)
FRAME_DTYPE = np.dtype([
    ("xpos", np.float32), ("ypos", np.float32), ("sigma", np.float32), ("orientation", np.float32),
    ("octave", np.int32), ("level", np.int32),
])
ORI_COMPUTE, ORI_GIVEN = 0, 1
FRAME_SIGMA_MAX = np.float32(8.0)  # POPSIFT_HIP_FRAME_SIGMA_MAX: the largest accepted scale in octave units

# every symbol include/popsift_hip.h declares: (name, restype, argtypes)
_vp, _ip = C.c_void_p, C.POINTER(C.c_int)
SYMBOLS = [
    ("popsift_hip_default_params", None, [C.POINTER(Params)]),
    ("popsift_hip_version", C.c_char_p, []),
    ("popsift_hip_strerror", C.c_char_p, [C.c_int]),
    ("popsift_hip_last_error", C.c_char_p, [_vp]),
    ("popsift_hip_device_count", C.c_int, [_ip]),
    ("popsift_hip_get_device_info", C.c_int, [C.c_int, C.POINTER(DeviceInfo)]),
    ("popsift_hip_device_numa_node", C.c_int, [C.c_int, _ip]),
    ("popsift_hip_plan_arena", C.c_int, [C.POINTER(Params), C.c_int, C.c_int, _ip, C.POINTER(C.c_int64)]),
    ("popsift_hip_ctx_create", C.c_int, [C.c_int, C.POINTER(Params), C.POINTER(_vp)]),
    ("popsift_hip_ctx_destroy", C.c_int, [_vp]),
    ("popsift_hip_get_gauss_table", C.c_int, [_vp, _vp, _vp, _vp, _ip]),
    ("popsift_hip_get_gauss_table_abs0", C.c_int, [_vp, _vp, _vp, _vp, _ip]),
    ("popsift_hip_get_gauss_table_dd", C.c_int, [_vp, _vp, _vp, _vp, _ip]),
    ("popsift_hip_submit_u8", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_f32", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_dev_u8", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_dev_f32", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_pinned_u8", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_pinned_f32", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_batch", C.c_int, [_vp, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_submit_batch_masked", C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_describe_batch", C.c_int, [_vp, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("popsift_hip_wait_batch", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("popsift_hip_fetch_item", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_results_dev_item", C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("popsift_hip_fetch_begin_item", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_set_keep_strongest", C.c_int, [_vp, C.c_int]),
    ("popsift_hip_fetch_responses_item", C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    ("popsift_hip_responses_dev_item", C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p)]),
    ("popsift_hip_wait", C.c_int, [_vp, _ip, _ip]),
    ("popsift_hip_fetch", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_fetch_begin", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_fetch_end", C.c_int, [_vp]),
    ("popsift_hip_results_dev", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    ("popsift_hip_fetch_item_u8", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_fetch_u8", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_fetch_begin_item_u8", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_fetch_begin_u8", C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t]),
    ("popsift_hip_results_dev_item_u8", C.c_int, [_vp, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("popsift_hip_host_alloc", _vp, [C.c_size_t]),
    ("popsift_hip_host_free", None, [_vp]),
    ("popsift_hip_clone_results", C.c_int, [_vp, C.POINTER(_vp)]),
    ("popsift_hip_devfeatures_free", C.c_int, [_vp]),
    ("popsift_hip_devfeatures_info", C.c_int, [_vp, _ip, _ip, _ip]),
    ("popsift_hip_devfeatures_ptrs", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    ("popsift_hip_devfeatures_alloc", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_devfeatures_from_host", C.c_int, [C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_devfeatures_download", C.c_int, [_vp, _vp, _vp]),
    ("popsift_hip_devfeatures_download_u8", C.c_int, [_vp, _vp]),
    ("popsift_hip_match_sets", C.c_int, [_vp, _vp, _vp]),
    ("popsift_hip_match_set_path", C.c_int, [C.c_int]),
    ("popsift_hip_devfeatures_debug_redo_count", C.c_int, [_vp, _ip]),
    ("popsift_hip_default_match_opts", None, [C.POINTER(MatchOpts)]),
    ("popsift_hip_match_pairs", C.c_int, [_vp, _vp, C.POINTER(MatchOpts), _vp, C.c_size_t, _ip]),
    ("popsift_hip_bytefeatures_from_host", C.c_int, [C.c_int, _vp, C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_bytefeatures_from_set", C.c_int, [_vp, C.POINTER(_vp)]),
    ("popsift_hip_clone_results_u8", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_bytefeatures_free", C.c_int, [_vp]),
    ("popsift_hip_bytefeatures_info", C.c_int, [_vp, _ip, _ip]),
    ("popsift_hip_bytefeatures_download", C.c_int, [_vp, _vp, _vp]),
    ("popsift_hip_match_bytes", C.c_int, [_vp, _vp, _vp]),
    ("popsift_hip_match_pairs_bytes", C.c_int, [_vp, _vp, C.POINTER(MatchOpts), _vp, C.c_size_t, _ip]),
    ("popsift_hip_gallery_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_gallery_free", C.c_int, [_vp]),
    ("popsift_hip_gallery_add", C.c_int, [_vp, _vp, _ip]),
    ("popsift_hip_gallery_add_host", C.c_int, [_vp, _vp, C.c_int, _ip]),
    ("popsift_hip_gallery_add_set", C.c_int, [_vp, _vp, _ip]),
    ("popsift_hip_gallery_pair_points", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("popsift_hip_gallery_info", C.c_int, [_vp, _ip, _ip, C.POINTER(C.c_int64)]),
    ("popsift_hip_gallery_member", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64), _ip]),
    ("popsift_hip_gallery_download", C.c_int, [_vp, C.c_int, _vp]),
    ("popsift_hip_gallery_debug_set_group_rows", C.c_int, [_vp, C.c_int]),
    ("popsift_hip_match_gallery", C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    ("popsift_hip_match_pairs_gallery", C.c_int, [_vp, _vp, C.POINTER(MatchOpts), _vp, C.c_size_t, _vp, _ip]),
    ("popsift_hip_match_links", C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t]),
    ("popsift_hip_match_pairs_links", C.c_int, [_vp, _vp, C.c_int, C.POINTER(MatchOpts), _vp, C.c_size_t, _vp, _ip]),
    ("popsift_hip_gallery_link_points", C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    ("popsift_hip_verifier_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_verifier_free", C.c_int, [_vp]),
    ("popsift_hip_default_ransac_opts", None, [C.POINTER(RansacOpts)]),
    ("popsift_hip_ransac", C.c_int, [_vp, _vp, C.c_int, C.POINTER(RansacOpts), _vp, _vp]),
    ("popsift_hip_ransac_trace", C.c_int, [_vp, _vp, C.c_int, C.POINTER(RansacOpts), _vp, _vp, _vp]),
    ("popsift_hip_pair_points", C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    ("popsift_hip_default_epipolar_opts", None, [C.POINTER(EpipolarOpts)]),
    ("popsift_hip_epipolar", C.c_int, [_vp, _vp, C.c_int, C.POINTER(EpipolarOpts), _vp, _vp]),
    ("popsift_hip_epipolar_trace", C.c_int, [_vp, _vp, C.c_int, C.POINTER(EpipolarOpts), _vp, _vp, _vp]),
    ("popsift_hip_default_refit_opts", None, [C.POINTER(RefitOpts)]),
    ("popsift_hip_refit", C.c_int, [_vp, _vp, C.c_int, C.POINTER(RefitOpts), _vp, _vp]),
    ("popsift_hip_refit_trace", C.c_int, [_vp, _vp, C.c_int, C.POINTER(RefitOpts), _vp, _vp, _vp, _vp, _vp, _vp]),
    ("popsift_hip_default_ransac_many_opts", None, [C.POINTER(RansacManyOpts)]),
    ("popsift_hip_ransac_many", C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(RansacManyOpts), _vp, _vp]),
    ("popsift_hip_ransac_many_trace", C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(RansacManyOpts), _vp, _vp, _vp, _vp, _vp]),
    ("popsift_hip_verifier_debug_set_group", C.c_int, [_vp, C.c_int]),
    ("popsift_hip_default_guided_opts", None, [C.POINTER(GuidedOpts)]),
    ("popsift_hip_match_guided", C.c_int, [_vp, _vp, C.POINTER(GuidedOpts), _vp]),
    ("popsift_hip_match_pairs_guided", C.c_int, [_vp, _vp, C.POINTER(GuidedOpts), _vp, C.c_size_t, _ip]),
    ("popsift_hip_devfeatures_from_host_points", C.c_int, [C.c_int, _vp, _vp, C.c_int, C.POINTER(_vp)]),
    ("popsift_hip_get_report", C.c_int, [_vp, C.POINTER(Report)]),
    ("popsift_hip_set_profile", C.c_int, [_vp, C.c_int]),
    ("popsift_hip_octave_dims", C.c_int, [_vp, C.c_int, _ip, _ip]),
    ("popsift_hip_download_plane", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("popsift_hip_upload_plane", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("popsift_hip_download_extrema", C.c_int, [_vp, _vp, C.c_size_t, _ip]),
    ("popsift_hip_rerun_keypoint_stages", C.c_int, [_vp]),
    ("popsift_hip_debug_set", C.c_int, [_vp, C.c_int, C.c_int]),
]
MATCH_AUTO, MATCH_EXACT, MATCH_SCREEN = 0, 1, 2
STAGES = ("pyramid", "detect", "refine", "orientation", "scan", "descriptor")
DEBUG_DET_QCAP, DEBUG_CAND_CAP, DEBUG_OHIST_CAP, DEBUG_FAIL_ALLOC, DEBUG_DESC_ROWS, DEBUG_KP_WAVES = 1, 2, 3, 4, 5, 7  # 6: retired
DEBUG_BLUR_PATH, DEBUG_BLUR_SEG, DEBUG_PYR_TAIL, DEBUG_DIRECT_PATH, DEBUG_DESC_CAP = 8, 9, 10, 11, 12
DEBUG_SCALE_PATH, DEBUG_ORDER_COARSE, DEBUG_DESC_LIST, DEBUG_BLUR_TILE_H = 13, 14, 15, 16
MAX_BATCH = 16
IMG_HOST_U8, IMG_HOST_F32, IMG_DEV_U8, IMG_DEV_F32, IMG_PINNED_U8, IMG_PINNED_F32 = range(6)

_lib = None


def _desc_type(fmt):
    """numpy element type of a descriptor format: "f32" (the default) or "u8" (popsift_hip_fetch*_u8)"""
    if fmt == "f32":
        return np.float32
    if fmt == "u8":
        return np.uint8
    raise ValueError("fmt: 'f32' or 'u8', got %r" % (fmt,))


def quantize_u8(desc):
    """The byte rule of popsift_hip_fetch_item_u8 on the host (the reference the tests hold the GPU pass to):
    0 for NaN and d <= 0, 255 for d >= 255, else roundf(d) -- ties away from zero -- as a byte."""
    d = np.asarray(desc, np.float32)
    with np.errstate(invalid="ignore"):
        pos = d > 0
        t = np.trunc(d)
        # roundf: |d - trunc(d)| >= 0.5 moves one away from zero (exact in float32 below 2^23)
        r = np.where(np.abs(d - t) >= np.float32(0.5), t + np.float32(1.0), t)
        r = np.where(d >= np.float32(255.0), np.float32(255.0), r)
        r = np.where(pos, r, np.float32(0.0))
    return r.astype(np.uint8)


class PopsiftHipError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = "%s failed: %d (%s)" % (where, status, lib().popsift_hip_strerror(status).decode())
        if detail:
            msg += ": " + detail
        super().__init__(msg)


def lib():
    """Load libpopsift_hip.so; raises if it is missing (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def default_params(**kw):
    p = Params()
    lib().popsift_hip_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def plan_arena(w, h, params=None):
    """(status, octaves, bytes of one image's plane arena) of a w x h image; needs no GPU.  The status is ERR_INVALID
    for an image a submit would refuse (empty, a side above 32767 after scaling, an arena of 4 GiB or more)."""
    p = params if params is not None else default_params()
    n, b = C.c_int(0), C.c_int64(0)
    rc = lib().popsift_hip_plan_arena(C.byref(p), w, h, C.byref(n), C.byref(b))
    return rc, n.value, b.value


def device_count():
    n = C.c_int(0)
    rc = lib().popsift_hip_device_count(C.byref(n))
    return n.value if rc == OK else 0


def device_info(device=0):
    d = DeviceInfo()
    rc = lib().popsift_hip_get_device_info(device, C.byref(d))
    if rc != OK:
        raise PopsiftHipError(rc, "popsift_hip_get_device_info")
    return d


class DevFeatures:
    """popsift_hip_devfeatures: a device-resident result set (FeaturesDev, features.h:98-118)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, desc, device=0):
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        h = _vp()
        rc = lib().popsift_hip_devfeatures_from_host(device, desc.ctypes.data, len(desc), C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_devfeatures_from_host")
        return cls(h)

    @classmethod
    def from_host_points(cls, desc, xy, device=0):
        """popsift_hip_devfeatures_from_host_points: descriptors (n, 128) with their positions (n, 2), one feature each"""
        desc = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        if len(xy) != len(desc):
            raise ValueError("from_host_points: %d descriptors, %d positions" % (len(desc), len(xy)))
        h = _vp()
        rc = lib().popsift_hip_devfeatures_from_host_points(device, desc.ctypes.data, xy.ctypes.data, len(desc), C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_devfeatures_from_host_points")
        return cls(h)

    def info(self):
        d, nf, nd = C.c_int(), C.c_int(), C.c_int()
        lib().popsift_hip_devfeatures_info(self._h, C.byref(d), C.byref(nf), C.byref(nd))
        return d.value, nf.value, nd.value

    def download(self):
        _, _, nd = self.info()
        desc = np.zeros((nd, 128), np.float32)
        rev = np.zeros(nd, np.int32)
        rc = lib().popsift_hip_devfeatures_download(self._h, desc.ctypes.data, rev.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_devfeatures_download")
        return desc, rev

    def download_u8(self):
        """the set's descriptors as bytes (n, 128), quantized on its GPU (popsift_hip_devfeatures_download_u8)"""
        _, _, nd = self.info()
        desc = np.zeros((nd, 128), np.uint8)
        rc = lib().popsift_hip_devfeatures_download_u8(self._h, desc.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_devfeatures_download_u8")
        return desc

    def match(self, other):
        _, _, nd = self.info()
        out = np.zeros(nd, MATCH_DTYPE)
        rc = lib().popsift_hip_match_sets(self._h, other._h, out.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_sets")
        return out

    def debug_redo_count(self):
        """Test hook (popsift_hip_devfeatures_debug_redo_count): rows the last forward screened sweep with this set on
        the left gave to the exact kernel; -1 before the first such sweep"""
        n = C.c_int(0)
        rc = lib().popsift_hip_devfeatures_debug_redo_count(self._h, C.byref(n))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_devfeatures_debug_redo_count")
        return n.value

    def match_pairs(self, other, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """Correspondences (popsift_hip_match_pairs): the rows of match(other) that pass the ratio test (0: none), the cap
        on the squared distance and, with cross_check, the mutual-nearest-neighbour check, as a PAIR_DTYPE array in
        ascending l.  Filtered on the GPU; only the pairs are downloaded."""
        _, _, nd = self.info()
        out = np.zeros(nd, PAIR_DTYPE)
        opts = MatchOpts(ratio, max_dist2, 1 if cross_check else 0, 0)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs(self._h, other._h, C.byref(opts), out.ctypes.data if nd else None, nd, C.byref(n))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_pairs")
        return out[:n.value]

    def match_guided(self, other, model, M, max_err=2.0):
        """popsift_hip_match_guided: a MATCH_DTYPE row per descriptor, its two nearest among the descriptors of `other`
        whose positions agree with the 3 x 3 model M (by name or number: homography / affine / epipolar) within max_err
        pixels; best / second are -1 where there is none"""
        _, _, nd = self.info()
        out = np.zeros(nd, MATCH_DTYPE)
        opts = guided_opts(model, M, max_err)
        rc = lib().popsift_hip_match_guided(self._h, other._h, C.byref(opts), out.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_guided")
        return out

    def match_pairs_guided(self, other, model, M, max_err=2.0, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """popsift_hip_match_pairs_guided: match_pairs' rule on match_guided's rows, as a PAIR_DTYPE array in ascending l"""
        _, _, nd = self.info()
        out = np.zeros(nd, PAIR_DTYPE)
        opts = guided_opts(model, M, max_err, ratio, max_dist2, cross_check)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs_guided(self._h, other._h, C.byref(opts), out.ctypes.data if nd else None, nd,
                                                  C.byref(n))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_guided")
        return out[:n.value]

    def pair_points(self, other, pairs):
        """popsift_hip_pair_points: (x, y, x', y') of each pair of match_pairs(other) as an (n, 4) float32 array, gathered on
        the GPU through the sets' descriptor -> feature maps; the input of Verifier.ransac"""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        pts = np.zeros((len(pairs), 4), np.float32)
        rc = lib().popsift_hip_pair_points(self._h, other._h, pairs.ctypes.data if len(pairs) else None, len(pairs),
                                           pts.ctypes.data if len(pairs) else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_pair_points")
        return pts

    def close(self):
        if self._h:
            lib().popsift_hip_devfeatures_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ByteFeatures:
    """popsift_hip_bytefeatures: a device-resident set of byte descriptors and its exact integer matcher."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, desc, device=0):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 128)
        h = _vp()
        rc = lib().popsift_hip_bytefeatures_from_host(device, desc.ctypes.data, len(desc), C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_bytefeatures_from_host")
        return cls(h)

    @classmethod
    def from_set(cls, features):
        """a DevFeatures set quantized on its GPU (the byte rule of popsift_hip_fetch_item_u8)"""
        h = _vp()
        rc = lib().popsift_hip_bytefeatures_from_set(features._h, C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_bytefeatures_from_set")
        return cls(h)

    def info(self):
        """(device, n_descriptors)"""
        d, nd = C.c_int(), C.c_int()
        lib().popsift_hip_bytefeatures_info(self._h, C.byref(d), C.byref(nd))
        return d.value, nd.value

    def download(self):
        """(desc (n, 128) uint8, descriptor -> feature map (n,) int32)"""
        nd = self.info()[1]
        desc = np.zeros((nd, 128), np.uint8)
        rev = np.zeros(nd, np.int32)
        rc = lib().popsift_hip_bytefeatures_download(self._h, desc.ctypes.data, rev.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_bytefeatures_download")
        return desc, rev

    def match(self, other):
        """popsift_hip_match_bytes: a MATCH_DTYPE row per descriptor; the distances are integers held in floats"""
        out = np.zeros(self.info()[1], MATCH_DTYPE)
        rc = lib().popsift_hip_match_bytes(self._h, other._h, out.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_bytes")
        return out

    def match_pairs(self, other, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """popsift_hip_match_pairs_bytes: DevFeatures.match_pairs' rule on match()'s rows; max_dist2 in byte units squared"""
        nd = self.info()[1]
        out = np.zeros(nd, PAIR_DTYPE)
        opts = MatchOpts(ratio, max_dist2, 1 if cross_check else 0, 0)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs_bytes(self._h, other._h, C.byref(opts), out.ctypes.data if nd else None, nd,
                                                 C.byref(n))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_bytes")
        return out[:n.value]

    def close(self):
        if self._h:
            lib().popsift_hip_bytefeatures_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GALLERY_GROUP_ROWS = 1 << 22  # POPSIFT_HIP_GALLERY_GROUP_ROWS
# popsift_hip_link: an ordered pair of member indices of one gallery, left image a and right image b
LINK_DTYPE = np.dtype([("a", np.int32), ("b", np.int32)])


def as_links(links):
    """a LINK_DTYPE array of anything that holds (a, b) pairs"""
    if isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE:
        return np.ascontiguousarray(links).reshape(-1)
    return np.ascontiguousarray(np.asarray(links, np.int32).reshape(-1, 2)).view(LINK_DTYPE).reshape(-1)


def all_links(n):
    """every a < b of n members, a-major: exhaustive matching"""
    a, b = np.triu_indices(n, 1)
    return as_links(np.stack([a, b], axis=1))


def sequential_links(n, k):
    """(a, a + 1 .. a + k) for every member a of a sequence of n"""
    return as_links([(a, b) for a in range(n) for b in range(a + 1, min(a + k, n - 1) + 1)])


class Gallery:
    """popsift_hip_gallery: byte sets end to end on one GPU, matched against one query set in one pass."""

    def __init__(self, device=0):
        h = _vp()
        rc = lib().popsift_hip_gallery_create(device, C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_create")
        self._h = h

    def add(self, member):
        """a ByteFeatures set (copied on the device) or an (n, 128) uint8 array; returns the member's index"""
        m = C.c_int(-1)
        if isinstance(member, ByteFeatures):
            rc, where = lib().popsift_hip_gallery_add(self._h, member._h, C.byref(m)), "popsift_hip_gallery_add"
        else:
            desc = np.ascontiguousarray(member, np.uint8).reshape(-1, 128)
            rc = lib().popsift_hip_gallery_add_host(self._h, desc.ctypes.data if len(desc) else None, len(desc), C.byref(m))
            where = "popsift_hip_gallery_add_host"
        if rc != OK:
            raise PopsiftHipError(rc, where)
        return m.value

    def add_set(self, features):
        """popsift_hip_gallery_add_set: a member from a DevFeatures set -- the bytes of ByteFeatures.from_set(features) and
        the positions behind its descriptors, for pair_points(); returns the member's index"""
        m = C.c_int(-1)
        rc = lib().popsift_hip_gallery_add_set(self._h, features._h, C.byref(m))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_add_set")
        return m.value

    def pair_points(self, query_set, pairs, offsets):
        """popsift_hip_gallery_pair_points: (n, 4) float32 rows (x, y, x', y') of the CSR (pairs, offsets) of match_pairs();
        query_set is the DevFeatures set the query bytes came from.  With the same offsets, the input of
        Verifier.ransac_many"""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(offsets) != self.info()[1] + 1 or offsets[-1] != len(pairs):
            raise ValueError("offsets: n_members + 1 ints, offsets[-1] = len(pairs)")
        pts = np.zeros((len(pairs), 4), np.float32)
        rc = lib().popsift_hip_gallery_pair_points(query_set._h, self._h, pairs.ctypes.data if len(pairs) else None,
                                                   offsets.ctypes.data, pts.ctypes.data if len(pairs) else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_pair_points")
        return pts

    def info(self):
        """(device, n_members, n_descriptors)"""
        d, nm, nd = C.c_int(), C.c_int(), C.c_int64()
        lib().popsift_hip_gallery_info(self._h, C.byref(d), C.byref(nm), C.byref(nd))
        return d.value, nm.value, nd.value

    def member(self, m):
        """(first descriptor, count) of member m"""
        first, count = C.c_int64(), C.c_int()
        rc = lib().popsift_hip_gallery_member(self._h, m, C.byref(first), C.byref(count))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_member")
        return first.value, count.value

    def download(self, m):
        """member m's bytes (count, 128)"""
        desc = np.zeros((self.member(m)[1], 128), np.uint8)
        rc = lib().popsift_hip_gallery_download(self._h, m, desc.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_download")
        return desc

    def match(self, query):
        """popsift_hip_match_gallery: (n_members, l_len) MATCH_DTYPE rows, row [m, i] = query.match(member m)[i]"""
        nm, nl = self.info()[1], query.info()[1]
        out = np.zeros((nm, nl), MATCH_DTYPE)
        rc = lib().popsift_hip_match_gallery(query._h, self._h, out.ctypes.data, nm * nl)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_gallery")
        return out

    def match_pairs(self, query, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """popsift_hip_match_pairs_gallery: (pairs, offsets); pairs[offsets[m]:offsets[m + 1]] = query.match_pairs(member m)"""
        nm, nl = self.info()[1], query.info()[1]
        out = np.zeros(nm * nl, PAIR_DTYPE)
        offsets = np.zeros(nm + 1, np.int32)
        opts = MatchOpts(ratio, max_dist2, 1 if cross_check else 0, 0)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs_gallery(query._h, self._h, C.byref(opts), out.ctypes.data if len(out) else None,
                                                   len(out), offsets.ctypes.data, C.byref(n))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_gallery")
        return out[:n.value], offsets

    def counts(self, query, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """pairs per member, without the pairs (cap = 0): which members match the query, and how strongly"""
        offsets = np.zeros(self.info()[1] + 1, np.int32)
        opts = MatchOpts(ratio, max_dist2, 1 if cross_check else 0, 0)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs_gallery(query._h, self._h, C.byref(opts), None, 0, offsets.ctypes.data, C.byref(n))
        if rc not in (OK, ERR_TOO_SMALL):                              # more pairs than cap = 0: the count is the answer
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_gallery")
        return np.diff(offsets)

    def _left_rows(self, links):
        """R[n_links]: the rows of match_links(), and a cap that always suffices for the pairs.  A left member out of range
        raises here as it would in the call."""
        counts = {int(a): self.member(int(a))[1] for a in np.unique(links["a"])}
        return sum(counts[int(a)] for a in links["a"])

    def match_links(self, links):
        """popsift_hip_match_links: the MATCH_DTYPE rows of every link, link after link; those of link e are member a_e
        matched against member b_e"""
        links = as_links(links)
        out = np.zeros(self._left_rows(links), MATCH_DTYPE)
        rc = lib().popsift_hip_match_links(self._h, links.ctypes.data if len(links) else None, len(links),
                                           out.ctypes.data if len(out) else None, len(out))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_links")
        return out

    def _pairs_links(self, links, cap, ratio, max_dist2, cross_check):
        out = np.empty(cap, PAIR_DTYPE)                                # the first n are written; untouched pages cost nothing
        offsets = np.zeros(len(links) + 1, np.int32)
        opts = MatchOpts(ratio, max_dist2, 1 if cross_check else 0, 0)
        n = C.c_int(0)
        rc = lib().popsift_hip_match_pairs_links(self._h, links.ctypes.data if len(links) else None, len(links), C.byref(opts),
                                                 out.ctypes.data if cap else None, cap, offsets.ctypes.data, C.byref(n))
        return rc, n.value, out, offsets

    def match_pairs_links(self, links, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """popsift_hip_match_pairs_links: (pairs, offsets); pairs[offsets[e]:offsets[e + 1]] is what the per-pair call returns
        for member a_e on the left and member b_e on the right"""
        links = as_links(links)
        rc, n, out, offsets = self._pairs_links(links, self._left_rows(links), ratio, max_dist2, cross_check)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_links")
        return out[:n].copy(), offsets

    def link_counts(self, links, ratio=0.8, max_dist2=np.inf, cross_check=False):
        """pairs per link, without the pairs (cap = 0): the edge weights of the view graph"""
        rc, _, _, offsets = self._pairs_links(as_links(links), 0, ratio, max_dist2, cross_check)
        if rc not in (OK, ERR_TOO_SMALL):                              # more pairs than cap = 0: the count is the answer
            raise PopsiftHipError(rc, "popsift_hip_match_pairs_links")
        return np.diff(offsets)

    def link_points(self, links, pairs, offsets):
        """popsift_hip_gallery_link_points: (n, 4) float32 rows (x, y, x', y') of the CSR (pairs, offsets) of
        match_pairs_links(), both positions from the members' own (add_set members).  With the same offsets, the input of
        Verifier.ransac_many"""
        links = as_links(links)
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(offsets) != len(links) + 1 or offsets[-1] != len(pairs):
            raise ValueError("offsets: n_links + 1 ints, offsets[-1] = len(pairs)")
        pts = np.zeros((len(pairs), 4), np.float32)
        rc = lib().popsift_hip_gallery_link_points(self._h, links.ctypes.data if len(links) else None, len(links),
                                                   pairs.ctypes.data if len(pairs) else None, offsets.ctypes.data,
                                                   pts.ctypes.data if len(pairs) else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_link_points")
        return pts

    def set_group_rows(self, n):
        """popsift_hip_gallery_debug_set_group_rows: rows of a group from the next call on; 0 = the default"""
        rc = lib().popsift_hip_gallery_debug_set_group_rows(self._h, n)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_gallery_debug_set_group_rows")

    def close(self):
        if self._h:
            lib().popsift_hip_gallery_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def guided_opts(model="homography", M=None, max_err=None, ratio=None, max_dist2=None, cross_check=None):
    """popsift_hip_guided_opts: the library's defaults with the given fields replaced; model by name or number, M any
    array of nine numbers in row-major order"""
    o = GuidedOpts()
    lib().popsift_hip_default_guided_opts(C.byref(o))
    o.model = GUIDES.get(model, model)
    if M is not None:
        o.M[:] = [float(v) for v in np.asarray(M, np.float32).reshape(9)]
    if max_err is not None:
        o.max_err = max_err
    if ratio is not None:
        o.ratio = ratio
    if max_dist2 is not None:
        o.max_dist2 = max_dist2
    if cross_check is not None:
        o.cross_check = 1 if cross_check else 0
    return o


def ransac_opts(model="homography", hypotheses=None, max_err=None, seed=None):
    """popsift_hip_ransac_opts: the library's defaults with the given fields replaced; model by name or number"""
    o = RansacOpts()
    lib().popsift_hip_default_ransac_opts(C.byref(o))
    o.model = MODELS.get(model, model)
    if hypotheses is not None:
        o.hypotheses = hypotheses
    if max_err is not None:
        o.max_err = max_err
    if seed is not None:
        o.seed = seed
    return o


def epipolar_opts(hypotheses=None, max_err=None, seed=None):
    """popsift_hip_epipolar_opts: the library's defaults with the given fields replaced"""
    o = EpipolarOpts()
    lib().popsift_hip_default_epipolar_opts(C.byref(o))
    if hypotheses is not None:
        o.hypotheses = hypotheses
    if max_err is not None:
        o.max_err = max_err
    if seed is not None:
        o.seed = seed
    return o


def refit_opts(model="homography", M=None, max_err=None, rounds=None):
    """popsift_hip_refit_opts: the library's defaults with the given fields replaced; model by name or number, M any array
    of nine numbers in row-major order"""
    o = RefitOpts()
    lib().popsift_hip_default_refit_opts(C.byref(o))
    o.model = REFITS.get(model, model)
    if M is not None:
        o.M[:] = [float(v) for v in np.asarray(M, np.float32).reshape(9)]
    if max_err is not None:
        o.max_err = max_err
    if rounds is not None:
        o.rounds = rounds
    return o


def ransac_many_opts(kind="homography", hypotheses=None, max_err=None, seed=None):
    """popsift_hip_ransac_many_opts: the library's defaults with the given fields replaced; kind by name or number"""
    o = RansacManyOpts()
    lib().popsift_hip_default_ransac_many_opts(C.byref(o))
    o.kind = REFITS.get(kind, kind)
    if hypotheses is not None:
        o.hypotheses = hypotheses
    if max_err is not None:
        o.max_err = max_err
    if seed is not None:
        o.seed = seed
    return o


class Verifier:
    """popsift_hip_verifier: RANSAC over point pairs on one GPU (a stream and grow-only scratch; one call at a time)."""

    def __init__(self, device=0):
        self._h = None
        h = _vp()
        rc = lib().popsift_hip_verifier_create(device, C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_verifier_create")
        self._h = h

    @staticmethod
    def _points(pts):
        pts = np.ascontiguousarray(pts, np.float32)
        if pts.size and (pts.ndim != 2 or pts.shape[1] != 4):
            raise ValueError("points: (n, 4) float32 rows (x, y, x', y')")
        return pts.reshape(-1, 4)

    def ransac(self, pts, model="homography", hypotheses=None, max_err=None, seed=None, want_mask=True):
        """popsift_hip_ransac -> (result, mask): result a RANSAC_RESULT_DTYPE record (H row major, n_inliers, hypothesis,
        n_valid), mask n bytes (None with want_mask=False)"""
        pts = self._points(pts)
        n = len(pts)
        res = np.zeros(1, RANSAC_RESULT_DTYPE)
        mask = np.zeros(n, np.uint8) if want_mask else None
        o = ransac_opts(model, hypotheses, max_err, seed)
        rc = lib().popsift_hip_ransac(self._h, pts.ctypes.data if n else None, n, C.byref(o), res.ctypes.data,
                                      mask.ctypes.data if want_mask and n else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_ransac")
        return res[0], mask

    def trace(self, pts, model="homography", hypotheses=None, max_err=None, seed=None):
        """popsift_hip_ransac_trace -> (samples (T, 4) int32, models (T, 9) float32, counts (T,) int32)"""
        pts = self._points(pts)
        n = len(pts)
        o = ransac_opts(model, hypotheses, max_err, seed)
        T = max(int(o.hypotheses), 0)
        samples, models, counts = np.zeros((T, 4), np.int32), np.zeros((T, 9), np.float32), np.zeros(T, np.int32)
        rc = lib().popsift_hip_ransac_trace(self._h, pts.ctypes.data if n else None, n, C.byref(o), samples.ctypes.data,
                                            models.ctypes.data, counts.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_ransac_trace")
        return samples, models, counts

    def epipolar(self, pts, hypotheses=None, max_err=None, seed=None, want_mask=True):
        """popsift_hip_epipolar -> (result, mask): as ransac(), with the fundamental matrix F in result["H"] (row major,
        [x' y' 1] F [x y 1]^T = 0) and max_err a Sampson distance"""
        pts = self._points(pts)
        n = len(pts)
        res = np.zeros(1, RANSAC_RESULT_DTYPE)
        mask = np.zeros(n, np.uint8) if want_mask else None
        o = epipolar_opts(hypotheses, max_err, seed)
        rc = lib().popsift_hip_epipolar(self._h, pts.ctypes.data if n else None, n, C.byref(o), res.ctypes.data,
                                        mask.ctypes.data if want_mask and n else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_epipolar")
        return res[0], mask

    def epipolar_trace(self, pts, hypotheses=None, max_err=None, seed=None):
        """popsift_hip_epipolar_trace -> (samples (T, 8) int32, models (T, 9) float32, counts (T,) int32)"""
        pts = self._points(pts)
        n = len(pts)
        o = epipolar_opts(hypotheses, max_err, seed)
        T = max(int(o.hypotheses), 0)
        samples, models, counts = (np.zeros((T, EPIPOLAR_SAMPLE), np.int32), np.zeros((T, 9), np.float32),
                                   np.zeros(T, np.int32))
        rc = lib().popsift_hip_epipolar_trace(self._h, pts.ctypes.data if n else None, n, C.byref(o), samples.ctypes.data,
                                              models.ctypes.data, counts.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_epipolar_trace")
        return samples, models, counts

    def refit(self, pts, model="homography", M=None, max_err=None, rounds=None, want_mask=True):
        """popsift_hip_refit -> (result, mask): the model M (of ransac() / epipolar(), or any other) fitted by least squares
        to its inliers, for up to `rounds` rounds; result a REFIT_RESULT_DTYPE record (M row major, n_inliers, n_start,
        rounds, stop), mask n bytes (None with want_mask=False)"""
        pts = self._points(pts)
        n = len(pts)
        res = np.zeros(1, REFIT_RESULT_DTYPE)
        mask = np.zeros(n, np.uint8) if want_mask else None
        o = refit_opts(model, M, max_err, rounds)
        rc = lib().popsift_hip_refit(self._h, pts.ctypes.data if n else None, n, C.byref(o), res.ctypes.data,
                                     mask.ctypes.data if want_mask and n else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_refit")
        return res[0], mask

    def refit_trace(self, pts, model="homography", M=None, max_err=None, rounds=None):
        """popsift_hip_refit_trace -> (result, mask, sums (rounds, 45) float64, models (rounds, 9) float32, counts (rounds,)
        int32, accepted (rounds,) int32)"""
        pts = self._points(pts)
        n = len(pts)
        res = np.zeros(1, REFIT_RESULT_DTYPE)
        mask = np.zeros(n, np.uint8)
        o = refit_opts(model, M, max_err, rounds)
        R = max(int(o.rounds), 0)
        sums, models = np.zeros((R, REFIT_SLOTS), np.float64), np.zeros((R, 9), np.float32)
        counts, accepted = np.zeros(R, np.int32), np.zeros(R, np.int32)
        rc = lib().popsift_hip_refit_trace(self._h, pts.ctypes.data if n else None, n, C.byref(o), res.ctypes.data,
                                           mask.ctypes.data if n else None, sums.ctypes.data, models.ctypes.data,
                                           counts.ctypes.data, accepted.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_refit_trace")
        return res[0], mask, sums, models, counts, accepted

    @staticmethod
    def _offsets(offsets, pts):
        offsets = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(offsets) < 1 or offsets[-1] != len(pts):
            raise ValueError("offsets: n_lists + 1 ints, offsets[0] = 0, offsets[-1] = len(pts)")
        return offsets

    def ransac_many(self, pts, offsets, kind="homography", hypotheses=None, max_err=None, seed=None, want_mask=True):
        """popsift_hip_ransac_many -> (results, mask): list m is pts[offsets[m]:offsets[m + 1]] (the CSR of
        Gallery.match_pairs / Gallery.pair_points); results (n_lists,) RANSAC_RESULT_DTYPE records, mask len(pts) bytes
        (None with want_mask=False), each list's what ransac() / epipolar() returns for it alone"""
        pts = self._points(pts)
        offsets = self._offsets(offsets, pts)
        nl, n = len(offsets) - 1, len(pts)
        res = np.zeros(nl, RANSAC_RESULT_DTYPE)
        mask = np.zeros(n, np.uint8) if want_mask else None
        o = ransac_many_opts(kind, hypotheses, max_err, seed)
        rc = lib().popsift_hip_ransac_many(self._h, pts.ctypes.data if n else None, offsets.ctypes.data, nl, C.byref(o),
                                           res.ctypes.data, mask.ctypes.data if want_mask and n else None)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_ransac_many")
        return res, mask

    def ransac_many_trace(self, pts, offsets, kind="homography", hypotheses=None, max_err=None, seed=None):
        """popsift_hip_ransac_many_trace -> (samples (n_lists, T, 4 | 8) int32, models (n_lists, T, 9) float32, counts
        (n_lists, T) int32)"""
        pts = self._points(pts)
        offsets = self._offsets(offsets, pts)
        nl, n = len(offsets) - 1, len(pts)
        o = ransac_many_opts(kind, hypotheses, max_err, seed)
        T = max(int(o.hypotheses), 0)
        row = EPIPOLAR_SAMPLE if o.kind == REFIT_EPIPOLAR else 4
        samples, models, counts = np.zeros((nl, T, row), np.int32), np.zeros((nl, T, 9), np.float32), np.zeros((nl, T), np.int32)
        rc = lib().popsift_hip_ransac_many_trace(self._h, pts.ctypes.data if n else None, offsets.ctypes.data, nl, C.byref(o),
                                                 None, None, samples.ctypes.data, models.ctypes.data, counts.ctypes.data)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_ransac_many_trace")
        return samples, models, counts

    def set_group(self, records):
        """popsift_hip_verifier_debug_set_group: (list, hypothesis) records of a group of ransac_many from the next call
        on; 0 = the default"""
        rc = lib().popsift_hip_verifier_debug_set_group(self._h, records)
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_verifier_debug_set_group")

    def close(self):
        if self._h:
            lib().popsift_hip_verifier_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PendingFetch:
    """A download started by Context.fetch_begin; result() waits for it (popsift_hip_fetch_end)."""

    def __init__(self, ctx, nf, nd, pinned, k=None, fmt="f32"):
        self._ctx, self._done = ctx, False
        dt = np.dtype(_desc_type(fmt))
        self._fbytes, self._dbytes = max(nf, 1) * FEATURE_DTYPE.itemsize, max(nd, 1) * 128 * dt.itemsize
        self._pin = []
        if pinned:
            for n in (self._fbytes, self._dbytes):
                p = lib().popsift_hip_host_alloc(n)
                if not p:
                    self._release()
                    raise MemoryError("popsift_hip_host_alloc(%d)" % n)
                self._pin.append(p)
            fb = (C.c_char * self._fbytes).from_address(self._pin[0])
            db = (C.c_char * self._dbytes).from_address(self._pin[1])
            self._feats = np.frombuffer(fb, FEATURE_DTYPE, nf)
            self._desc = np.frombuffer(db, dt, nd * 128).reshape(nd, 128)
        else:
            self._feats = np.zeros(nf, FEATURE_DTYPE)
            self._desc = np.zeros((nd, 128), dt)
        try:
            f, d = self._feats.ctypes.data, self._desc.ctypes.data
            if k is None:
                fn = lib().popsift_hip_fetch_begin_u8 if fmt == "u8" else lib().popsift_hip_fetch_begin
                rc = fn(ctx._h, f, nf, d, nd * 128)
            else:
                fn = lib().popsift_hip_fetch_begin_item_u8 if fmt == "u8" else lib().popsift_hip_fetch_begin_item
                rc = fn(ctx._h, k, f, nf, d, nd * 128)
            ctx._chk(rc, "popsift_hip_fetch_begin")
        except Exception:
            self._release()
            raise

    def _release(self):
        for p in self._pin:
            lib().popsift_hip_host_free(p)
        self._pin = []

    def _landed(self):
        """the download is complete (fetch_end, or a later fetch_begin on the same context, has waited for it)"""
        self._done = True
        if self._pin:
            self._feats, self._desc = self._feats.copy(), self._desc.copy()
            self._release()

    def result(self):
        """(feats, desc) as ordinary numpy arrays (copied out of the pinned blocks, which are released)."""
        if not self._done:
            rc = lib().popsift_hip_fetch_end(self._ctx._h)
            # ERR_STATE: nothing is pending any more -- a later fetch_begin on the context has already waited for this
            # download (popsift_hip_fetch_begin drains the previous one first, also when it then fails): the data is there
            if rc != ERR_STATE:
                self._ctx._chk(rc, "popsift_hip_fetch_end")
            self._landed()
        return self._feats, self._desc

    def __del__(self):
        try:
            if not self._done and self._ctx._h:
                lib().popsift_hip_fetch_end(self._ctx._h)
            self._release()
        except Exception:
            pass


class Context:
    """One extraction context (popsift_hip_ctx) on one GPU."""

    def __init__(self, params=None, device=0):
        self._h = None
        self.params = params if params is not None else default_params()
        h = _vp()
        rc = lib().popsift_hip_ctx_create(device, C.byref(self.params), C.byref(h))
        if rc != OK:
            raise PopsiftHipError(rc, "popsift_hip_ctx_create")
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            lib().popsift_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc != OK:
            raise PopsiftHipError(rc, where, lib().popsift_hip_last_error(self._h).decode())

    def gauss_table(self, abs0=False, dd=False):
        """(filter[L, 32], span[L], sigma[L]): the incremental table, or with abs0=True the abs_o0 table of the
        vlfeat-direct Gauss mode (octave 0's levels straight from the input image), or with dd=True the dd table of the
        ScaleDirect scaling mode (one row per octave: each octave's level 0 straight from the input image)"""
        if abs0 and dd:
            raise ValueError("abs0 or dd, not both")
        get = (lib().popsift_hip_get_gauss_table_abs0 if abs0 else
               lib().popsift_hip_get_gauss_table_dd if dd else lib().popsift_hip_get_gauss_table)
        n = C.c_int()
        self._chk(get(self._h, None, None, None, C.byref(n)), "get_gauss_table")
        f = np.zeros((n.value, 32), np.float32)
        s = np.zeros(n.value, np.int32)
        g = np.zeros(n.value, np.float32)
        self._chk(get(self._h, f.ctypes.data, s.ctypes.data, g.ctypes.data, C.byref(n)), "get_gauss_table")
        return f, s, g

    def submit(self, img, mask=None):
        """one host image; mask: a uint8 (H, W) array, non-zero = visible (popsift_hip_submit_batch_masked), or None"""
        if mask is not None:
            return self.submit_batch([img], [mask])
        img = np.ascontiguousarray(img)
        if img.ndim != 2:
            raise ValueError("grayscale (H, W) image expected")
        h, w = img.shape
        if img.dtype == np.uint8:
            rc = lib().popsift_hip_submit_u8(self._h, img.ctypes.data, w, h, w)
        elif img.dtype == np.float32:
            rc = lib().popsift_hip_submit_f32(self._h, img.ctypes.data, w, h, w)
        else:
            raise TypeError("uint8 or float32 image expected, got %s" % img.dtype)
        self._chk(rc, "popsift_hip_submit")
        return self

    def submit_pinned(self, ptr, w, h, pitch, is_f32=False):
        """image in page-locked host memory (host_alloc), uploaded without a staging copy; keep it until wait()"""
        fn = lib().popsift_hip_submit_pinned_f32 if is_f32 else lib().popsift_hip_submit_pinned_u8
        self._chk(fn(self._h, ptr, w, h, pitch), "popsift_hip_submit_pinned")
        return self

    def submit_dev(self, ptr, w, h, pitch, is_f32=False):
        fn = lib().popsift_hip_submit_dev_f32 if is_f32 else lib().popsift_hip_submit_dev_u8
        self._chk(fn(self._h, ptr, w, h, pitch), "popsift_hip_submit_dev")
        return self

    def submit_batch(self, imgs, masks=None):
        """popsift_hip_submit_batch: several host images of one size and dtype, extracted together.  masks: a list with a
        uint8 (H, W) array (non-zero = visible) or None per image (popsift_hip_submit_batch_masked)"""
        imgs = [np.ascontiguousarray(im) for im in imgs]
        if any(im.ndim != 2 for im in imgs):
            raise ValueError("grayscale (H, W) images expected")
        h, w = imgs[0].shape
        if any(im.shape != (h, w) or im.dtype != imgs[0].dtype for im in imgs):
            raise ValueError("the images of a batch share one size and dtype")
        if imgs[0].dtype == np.uint8:
            kind = IMG_HOST_U8
        elif imgs[0].dtype == np.float32:
            kind = IMG_HOST_F32
        else:
            raise TypeError("uint8 or float32 images expected, got %s" % imgs[0].dtype)
        arr = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        if masks is None:
            self._chk(lib().popsift_hip_submit_batch(self._h, arr, len(imgs), kind, w, h, w), "popsift_hip_submit_batch")
            return self
        if len(masks) != len(imgs):
            raise ValueError("one mask (or None) per image")
        masks = [None if m is None else np.ascontiguousarray(m) for m in masks]
        if any(m is not None and (m.shape != (h, w) or m.dtype != np.uint8) for m in masks):
            raise ValueError("a mask is a uint8 array of the image's size")
        marr = (C.c_void_p * len(imgs))(*[None if m is None else m.ctypes.data for m in masks])
        self._chk(lib().popsift_hip_submit_batch_masked(self._h, arr, marr, len(imgs), kind, w, h, w, w),
                  "popsift_hip_submit_batch_masked")
        return self

    def submit_batch_dev(self, ptrs, w, h, pitch, is_f32=False, masks=None, mask_pitch=None):
        """the same for images resident in this device's memory (ptrs: device addresses); masks: device addresses of the
        masks (or None entries) with rows mask_pitch bytes apart (default w)"""
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        kind = IMG_DEV_F32 if is_f32 else IMG_DEV_U8
        if masks is None:
            self._chk(lib().popsift_hip_submit_batch(self._h, arr, len(ptrs), kind, w, h, pitch), "popsift_hip_submit_batch")
            return self
        if len(masks) != len(ptrs):
            raise ValueError("one mask (or None) per image")
        marr = (C.c_void_p * len(ptrs))(*masks)
        self._chk(lib().popsift_hip_submit_batch_masked(self._h, arr, marr, len(ptrs), kind, w, h, pitch,
                                                         w if mask_pitch is None else mask_pitch),
                  "popsift_hip_submit_batch_masked")
        return self

    def describe_batch_async(self, imgs, frame_lists, orientation="compute"):
        """popsift_hip_describe_batch: host images of one size and dtype, each with its own FRAME_DTYPE frames; results as
        for submit_batch (wait_batch / fetch_item), one feature per frame in caller order"""
        if orientation not in ("compute", "given"):
            raise ValueError("orientation: 'compute' or 'given'")
        imgs = [np.ascontiguousarray(im) for im in imgs]
        if len(frame_lists) != len(imgs):
            raise ValueError("one frame list per image")
        h, w = imgs[0].shape
        if any(im.ndim != 2 or im.shape != (h, w) or im.dtype != imgs[0].dtype for im in imgs):
            raise ValueError("the images of a batch share one size and dtype")
        if imgs[0].dtype == np.uint8:
            kind = IMG_HOST_U8
        elif imgs[0].dtype == np.float32:
            kind = IMG_HOST_F32
        else:
            raise TypeError("uint8 or float32 images expected, got %s" % imgs[0].dtype)
        frs = [np.ascontiguousarray(f, FRAME_DTYPE) for f in frame_lists]
        arr = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        farr = (C.c_void_p * len(imgs))(*[f.ctypes.data if len(f) else None for f in frs])
        nfr = (C.c_int * len(imgs))(*[len(f) for f in frs])
        self._chk(lib().popsift_hip_describe_batch(self._h, arr, farr, nfr, len(imgs), kind, w, h, w,
                                                   ORI_GIVEN if orientation == "given" else ORI_COMPUTE),
                  "popsift_hip_describe_batch")
        return self

    def describe(self, img, frames, orientation="compute"):
        """descriptors of caller-supplied keypoints (FRAME_DTYPE) -> (feats, desc), feature i for frame i.
        orientation="compute": up to four orientations per frame as extraction finds them; "given": frames["orientation"]"""
        return self.describe_batch_async([img], [frames], orientation).fetch_item(0)

    def describe_batch(self, imgs, frame_lists, orientation="compute"):
        """-> [(feats, desc)] per image, as describe() gives them"""
        self.describe_batch_async(imgs, frame_lists, orientation)
        return [self.fetch_item(k) for k in range(len(imgs))]

    def wait_batch(self):
        """-> [(features, descriptors)] per image of the batch"""
        n = C.c_int()
        nf = (C.c_int * MAX_BATCH)()
        nd = (C.c_int * MAX_BATCH)()
        self._chk(lib().popsift_hip_wait_batch(self._h, C.byref(n), nf, nd), "popsift_hip_wait_batch")
        return [(nf[k], nd[k]) for k in range(n.value)]

    def fetch_item(self, k, fmt="f32"):
        """(feats, desc) of image k of the finished batch; fmt="u8": descriptors as bytes, quantized on the GPU"""
        nf, nd = self.wait_batch()[k]
        feats = np.zeros(nf, FEATURE_DTYPE)
        desc = np.zeros((nd, 128), _desc_type(fmt))
        fn = lib().popsift_hip_fetch_item_u8 if fmt == "u8" else lib().popsift_hip_fetch_item
        self._chk(fn(self._h, k, feats.ctypes.data, nf, desc.ctypes.data, nd * 128), "popsift_hip_fetch_item")
        return feats, desc

    def fetch_begin_item(self, k, pinned=True, fmt="f32"):
        """fetch_begin for image k of the finished batch (call it for every image, submit the next batch, then result()
        of any one handle -- one popsift_hip_fetch_end -- completes them all)"""
        nf, nd = self.wait_batch()[k]
        return PendingFetch(self, nf, nd, pinned, k=k, fmt=fmt)

    def results_dev_item(self, k, fmt="f32"):
        """(device address of the features, of the descriptors) of image k; fmt="u8": the byte descriptors"""
        fp, dp = C.c_void_p(), C.c_void_p()
        fn = lib().popsift_hip_results_dev_item_u8 if fmt == "u8" else lib().popsift_hip_results_dev_item
        self._chk(fn(self._h, k, C.byref(fp), C.byref(dp)), "popsift_hip_results_dev_item")
        return fp.value, dp.value

    def wait(self):
        a, b = C.c_int(), C.c_int()
        self._chk(lib().popsift_hip_wait(self._h, C.byref(a), C.byref(b)), "popsift_hip_wait")
        return a.value, b.value

    def fetch(self, fmt="f32"):
        """(feats, desc) of the finished image; fmt="u8": descriptors as bytes, quantized on the GPU"""
        nf, nd = self.wait()
        feats = np.zeros(nf, FEATURE_DTYPE)
        desc = np.zeros((nd, 128), _desc_type(fmt))
        fn = lib().popsift_hip_fetch_u8 if fmt == "u8" else lib().popsift_hip_fetch
        self._chk(fn(self._h, feats.ctypes.data, nf, desc.ctypes.data, nd * 128), "popsift_hip_fetch")
        return feats, desc

    def fetch_begin(self, pinned=True, fmt="f32"):
        """Start the download of the finished image and return a handle; the context is free for the next submit.
        handle.result() (popsift_hip_fetch_end) -> (feats, desc).  pinned: page-locked targets (asynchronous copy).
        fmt="u8": descriptors as bytes, quantized on the GPU."""
        nf, nd = self.wait()
        prev = getattr(self, "_pending", None)
        self._pending = PendingFetch(self, nf, nd, pinned, fmt=fmt)   # the C call waits for an earlier pending download first
        if prev is not None and not prev._done:
            prev._landed()
        return self._pending

    def report(self):
        r = Report()
        self._chk(lib().popsift_hip_get_report(self._h, C.byref(r)), "popsift_hip_get_report")
        return r

    def set_profile(self, mode):
        """0 off, 1 (True): every blur launch timed, 2: stage times (report().ms_stage)"""
        self._chk(lib().popsift_hip_set_profile(self._h, int(mode)), "popsift_hip_set_profile")

    def set_keep_strongest(self, n):
        """popsift_hip_set_keep_strongest: from the next submit (or rerun_keypoint_stages) keep the n keypoints of every
        image with the largest DoG response, ties with the n-th included (tests/strongest_rule.py states the rule);
        0 = off.  A huge n (2**31 - 1) thins nothing and still makes fetch_responses work."""
        self._chk(lib().popsift_hip_set_keep_strongest(self._h, int(n)), "popsift_hip_set_keep_strongest")
        return self

    def fetch_responses(self, k=0):
        """the response of every feature of image k of the finished batch (float32, feature order); needs
        set_keep_strongest(n > 0) at the submit"""
        nf = self.wait_batch()[k][0]
        out = np.zeros(nf, np.float32)
        self._chk(lib().popsift_hip_fetch_responses_item(self._h, k, out.ctypes.data, nf), "popsift_hip_fetch_responses_item")
        return out

    def octave_dims(self, o):
        w, h = C.c_int(), C.c_int()
        self._chk(lib().popsift_hip_octave_dims(self._h, o, C.byref(w), C.byref(h)), "popsift_hip_octave_dims")
        return w.value, h.value

    def plane(self, octave, kind, level):
        w, h = self.octave_dims(octave)
        out = np.zeros((h, w), np.float32)
        self._chk(lib().popsift_hip_download_plane(self._h, octave, kind, level, out.ctypes.data), "download_plane")
        return out

    def upload_plane(self, octave, kind, level, arr):
        w, h = self.octave_dims(octave)
        arr = np.ascontiguousarray(arr, np.float32)
        assert arr.shape == (h, w)
        self._chk(lib().popsift_hip_upload_plane(self._h, octave, kind, level, arr.ctypes.data), "upload_plane")

    def extrema(self):
        n = C.c_int()
        self._chk(lib().popsift_hip_download_extrema(self._h, None, 0, C.byref(n)), "download_extrema")
        out = np.zeros(n.value, EXTREMUM_DTYPE)
        self._chk(lib().popsift_hip_download_extrema(self._h, out.ctypes.data, n.value, C.byref(n)),
                  "download_extrema")
        return out

    def clone_results(self):
        h = _vp()
        self._chk(lib().popsift_hip_clone_results(self._h, C.byref(h)), "popsift_hip_clone_results")
        return DevFeatures(h)

    def clone_results_u8(self, k=0):
        """image k's descriptors as a device-resident byte set (popsift_hip_clone_results_u8)"""
        h = _vp()
        self._chk(lib().popsift_hip_clone_results_u8(self._h, k, C.byref(h)), "popsift_hip_clone_results_u8")
        return ByteFeatures(h)

    def rerun_keypoint_stages(self):
        self._chk(lib().popsift_hip_rerun_keypoint_stages(self._h), "rerun_keypoint_stages")
        return self

    def debug_set(self, what, value):
        """popsift_hip_debug_set: test switches (DEBUG_*), before the first submit"""
        self._chk(lib().popsift_hip_debug_set(self._h, what, value), "popsift_hip_debug_set")
        return self
