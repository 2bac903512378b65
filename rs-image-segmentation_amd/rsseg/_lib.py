"""
ctypes binding of librsseg_hip.so (include/rsseg.h).  This is the only place the C ABI is declared
on the Python side.  Loading fails loudly: there is no CPU fallback for the product path.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "librsseg_hip.so")

MAX_FEATURES = 64
MAX_CLUSTERS = 64
MAX_RANKS = 16
F32, F64, I64 = 0, 1, 2
U8, I16, U16, I32 = 3, 4, 5, 6   # integer label planes (rsseg_confusion_counts), DN planes (rsseg_preprocess_u8)
EVAL_MAX_CELLS = 4096            # the largest table rsseg_confusion_counts builds on the device
SUM, MIN, MAX = 0, 1, 2
BORDER_REFLECT, BORDER_REFLECT101 = 0, 1
MORPH_ERODE, MORPH_DILATE, MORPH_OPEN, MORPH_CLOSE, MORPH_GRADIENT = 0, 1, 2, 3, 4
MASK_AND, MASK_OR, MASK_ANDNOT, MASK_NOT = 0, 1, 2, 3
VALID_NAN, VALID_INF, VALID_VALUE = 1, 2, 4   # rsseg_valid_mask's flags
WARP_NEAREST, WARP_BILINEAR, WARP_CUBIC = 0, 1, 2
WARP_MAX_BANDS = 16
OBJ_GEOMETRY = 1   # rsseg_segment_features' flag

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int)


class KMeansInfo(C.Structure):
    _fields_ = [
        ("n_iter", C.c_int32),
        ("relocated", C.c_int32),
        ("tol", C.c_double),
        ("scale", C.c_double * MAX_FEATURES),
        ("min", C.c_double * MAX_FEATURES),
        ("mean", C.c_double * MAX_FEATURES),
        ("init_indices", C.c_int64 * MAX_CLUSTERS),
        ("ms_init", C.c_double),
        ("ms_lloyd", C.c_double),
    ]


class KMeansApplyInfo(C.Structure):
    _fields_ = [
        ("counts", C.c_int64 * MAX_CLUSTERS),
        ("inertia", C.c_double),
        ("overflow", C.c_int32),
        ("ms", C.c_double),
    ]


# rsseg_forest_job of include/rsseg.h as a NumPy record: one per tree of rsseg_forest_fit_jobs
FOREST_JOB = [("counts_row", "<i8"), ("weight_total", "<i8"), ("seed", "<u4"), ("max_depth", "<i4"), ("min_samples_split", "<i4"),
              ("min_samples_leaf", "<i4"), ("max_features", "<i4"), ("reserved", "<i4")]
# rsseg_perm_job of include/rsseg.h: one per job of rsseg_forest_permutation_counts (feature -1: no substitution)
PERM_JOB = [("feature", "<i4"), ("source", "<i4")]

_vp = C.c_void_p
_i64 = C.c_int64
_int = C.c_int
_PP = C.POINTER(C.c_void_p)

# name -> (restype, argtypes); mirrors include/rsseg.h one to one
SIGNATURES = {
    "rsseg_ctx_create": (_int, [_int, _vp, C.POINTER(_vp)]),
    "rsseg_ctx_destroy": (None, [_vp]),
    "rsseg_last_error": (C.c_char_p, [_vp]),
    "rsseg_version": (C.c_char_p, []),
    "rsseg_ctx_set_comm": (_int, [_vp, _int, _int, ALLREDUCE_FN, _vp, _vp, C.c_size_t]),
    "rsseg_ctx_set_async": (_int, [_vp, _int]),
    "rsseg_ctx_sync": (_int, [_vp]),
    "rsseg_ctx_host_syncs": (_int, [_vp, _int, C.POINTER(_i64)]),
    "rsseg_prof_enable": (_int, [_vp, _int]),
    "rsseg_prof_reset": (_int, [_vp]),
    "rsseg_prof_get": (_int, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_i64)]),
    "rsseg_order_stats_f32": (_int, [_vp, _vp, _i64, C.POINTER(_i64), _int, C.POINTER(C.c_float), C.POINTER(_i64)]),
    "rsseg_order_stats_multi_f32": (_int, [_vp, C.POINTER(_vp), _int, _i64, C.POINTER(_i64), _int, C.POINTER(C.c_float), C.POINTER(_i64)]),
    "rsseg_order_stats_multi_u8": (_int, [_vp, C.POINTER(_vp), _int, _i64, C.POINTER(_i64), _int, C.POINTER(C.c_float), C.POINTER(_i64)]),
    "rsseg_spectral_indices_evi_u8": (_int, [_vp, _PP, _i64, C.POINTER(C.c_float), _PP, _PP, C.POINTER(C.c_float)]),
    "rsseg_pca_fit_transform_ext_u8": (_int, [_vp, _PP, _int, _i64, _i64, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                              _int, _PP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                              C.POINTER(C.c_float)]),
    "rsseg_indices_pca_f32": (_int, [_vp, _PP, _int, _i64, _i64, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double), _int,
                                     C.POINTER(C.c_float), _PP, _PP, _PP, _vp, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float),
                                     C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rsseg_indices_pca_u8": (_int, [_vp, _PP, _int, _i64, _i64, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double), _int,
                                    C.POINTER(C.c_float), _PP, _PP, _PP, _vp, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "rsseg_normalize_f32": (_int, [_vp, _vp, _i64, C.c_float, C.c_float, _vp]),
    "rsseg_spectral_indices_f32": (_int, [_vp, _PP, _i64, C.POINTER(C.c_float), _PP, _PP]),
    "rsseg_spectral_indices_evi_f32": (_int, [_vp, _PP, _i64, C.POINTER(C.c_float), _PP, _PP, C.POINTER(C.c_float)]),
    "rsseg_pca_fit_transform_f32": (_int, [_vp, _PP, _int, _i64, C.POINTER(C.c_float), C.POINTER(C.c_double), _int, _PP,
                                           C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           C.POINTER(C.c_float)]),
    "rsseg_pca_fit_transform_raw_f32": (_int, [_vp, _PP, _int, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                               _int, _PP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float)]),
    "rsseg_pca_fit_transform_ext_f32": (_int, [_vp, _PP, _int, _i64, _i64, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                               _int, _PP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                               C.POINTER(C.c_float)]),
    "rsseg_normalize_quantize_u8": (_int, [_vp, _vp, _i64, C.c_float, C.c_float, C.c_float, _vp]),
    "rsseg_glcm_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _PP]),
    "rsseg_glcm_offsets_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, C.POINTER(C.c_int32), _int, _PP]),
    "rsseg_quantize_u8": (_int, [_vp, _vp, _i64, C.c_float, _vp]),
    "rsseg_u8_to_unit_f32": (_int, [_vp, _vp, _i64, _vp]),
    "rsseg_u8_to_f32": (_int, [_vp, _vp, _i64, _vp]),
    "rsseg_resize_bilinear_f32": (_int, [_vp, _vp, _int, _int, _vp, _int, _int]),
    "rsseg_resize_bilinear_rows_f32": (_int, [_vp, _vp, _int, _int, _int, _int, _vp, _int, _int, _int, _int]),
    "rsseg_resize_bilinear_rows_multi_f32": (_int, [_vp, _PP, _int, _int, _int, _int, _int, _PP, _int, _int, _int, _int]),
    "rsseg_box_mean_f32": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _vp]),
    "rsseg_box_mean_rows_f32": (_int, [_vp, _PP, _int, _int, _int, _int, _int, _int, _int, _int, _int, _PP]),
    "rsseg_local_std_rows_f32": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "rsseg_morph_rows_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _int, _vp]),
    "rsseg_laplacian_norm_rows_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _vp]),
    "rsseg_sobel_mag_rows_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _vp]),
    "rsseg_local_std_f32": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_morph_gradient_u8": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_morph_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _vp]),
    "rsseg_local_var_f32": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_laplacian_norm_u8": (_int, [_vp, _vp, _int, _int, _vp]),
    "rsseg_sobel_mag_u8": (_int, [_vp, _vp, _int, _int, _vp]),
    "rsseg_correlate_u8_f32": (_int, [_vp, _vp, _int, _int, C.POINTER(C.c_float), _int, _int, _vp, C.POINTER(C.c_float)]),
    "rsseg_filter_bank_norm_u8": (_int, [_vp, _vp, _int, _int, C.POINTER(C.c_float), _int, _int, _vp]),
    "rsseg_correlate_tile": (None, [C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_kmeans_fit_predict": (_int, [_vp, _PP, _int, _int, _i64, _int, C.c_uint32, _int, C.c_double, _vp,
                                        C.POINTER(C.c_double), C.POINTER(KMeansInfo)]),
    "rsseg_kmeans_fit_predict_mm": (_int, [_vp, _PP, _int, _int, _i64, _int, C.c_uint32, _int, C.c_double, _vp,
                                           C.POINTER(C.c_double), C.POINTER(KMeansInfo), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rsseg_kmeans_predict": (_int, [_vp, _PP, _int, _int, _i64, _int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, _vp,
                                    C.POINTER(KMeansApplyInfo)]),
    "rsseg_gauss_classify": (_int, [_vp, _PP, _int, _int, _i64, _int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_uint8), C.c_double, _vp, _vp, _vp]),
    "rsseg_svm_classify": (_int, [_vp, _PP, _int, _int, _i64, _int, _int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8), _int, C.c_double,
                                  C.c_double, _int, C.POINTER(C.c_double), _vp, _vp]),
    "rsseg_host_svm_fold_linear": (_int, [_int, _int, _int, C.POINTER(C.c_double), C.POINTER(_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rsseg_mlp_classify": (_int, [_vp, _PP, _int, _i64, _int, C.POINTER(_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), _int, _int, C.POINTER(C.c_uint8), _vp, _vp, _vp, _vp]),
    "rsseg_mlp_plan": (None, [_int, _int, C.POINTER(_int), _int, C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_valid_mask": (_int, [_vp, _PP, _int, _int, _i64, _int, C.c_double, _vp, _vp, C.POINTER(_i64)]),
    "rsseg_compact_tile": (_int, []),
    "rsseg_compact_scan_span": (_int, []),
    "rsseg_compact_plan": (_int, [_vp, _vp, _i64, _vp, C.POINTER(_i64)]),
    "rsseg_compact_planes": (_int, [_vp, _vp, _vp, _i64, _PP, _int, _int, _PP]),
    "rsseg_expand_plane": (_int, [_vp, _vp, _vp, _i64, _vp, _int, _vp, _vp]),
    "rsseg_ctx_allreduce": (_int, [_vp, _i64, _i64, _int, _int]),
    "rsseg_rccl_unique_id": (_int, [C.c_char_p, _vp]),
    "rsseg_ctx_set_comm_rccl": (_int, [_vp, _int, _int, _vp, C.c_char_p, _vp, C.c_size_t]),
    "rsseg_ctx_collect_minmax": (_int, [_vp, _int]),
    "rsseg_ctx_last_minmax": (_int, [_vp, _int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rsseg_forest_load": (_int, [_vp, _int, C.POINTER(_i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                                 C.POINTER(C.c_double), _int, C.POINTER(_i64), _int]),
    "rsseg_forest_predict": (_int, [_vp, _PP, _int, _i64, _vp]),
    "rsseg_forest_predict_proba": (_int, [_vp, _PP, _int, _i64, _vp, _vp, _vp]),
    "rsseg_forest_oob": (_int, [_vp, _PP, _int, _i64, _vp, _vp, _vp]),
    "rsseg_forest_permutation_counts": (_int, [_vp, _PP, _int, _i64, _vp, _vp, _int, _vp, _int, C.POINTER(_i64)]),
    "rsseg_forest_fit": (_int, [_vp, _PP, _int, _i64, _vp, _int, _vp, _int, _int, C.POINTER(C.c_uint32), _int, _int, _int, _int,
                                C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64),
                                C.POINTER(C.c_int32)]),
    "rsseg_forest_fit_jobs": (_int, [_vp, _PP, _int, _i64, _vp, _int, _vp, _i64, _int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "rsseg_threshold_band_f32": (_int, [_vp, _vp, _i64, C.c_float, C.c_float, _vp]),
    "rsseg_band_interval_f32": (_int, [_vp, _vp, _i64, C.c_float, C.c_float, _int, _vp]),
    "rsseg_band_interval_f64": (_int, [_vp, _vp, _i64, C.c_double, C.c_double, _int, _vp]),
    "rsseg_otsu_mask": (_int, [_vp, _vp, _int, _i64, _int, _vp, C.POINTER(_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "rsseg_fill_holes_u8": (_int, [_vp, _vp, _int, _int, _vp]),
    "rsseg_mask_op_u8": (_int, [_vp, _vp, _vp, _i64, _int, _vp]),
    "rsseg_mask_paint_u8": (_int, [_vp, _vp, _vp, _i64, _int, _int]),
    "rsseg_morph_ellipse_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _vp]),
    "rsseg_remove_small_components_u8": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_hist_u8": (_int, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "rsseg_replace_u8": (_int, [_vp, _vp, _i64, _int, _int, C.POINTER(_i64)]),
    "rsseg_majority_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _int, _int, _int, _int, C.c_uint32, _vp, C.POINTER(_i64),
                                 C.POINTER(_i64)]),
    "rsseg_sieve_u8": (_int, [_vp, _vp, _int, _int, _int, _int, _int, _int, _vp, C.POINTER(_i64)]),
    "rsseg_slic_u8": (_int, [_vp, _PP, _int, _int, _int, _vp, _int, C.c_double, _int, _int, _vp, C.POINTER(_i64), C.POINTER(_int), C.POINTER(_i64)]),
    "rsseg_slic_tile": (None, [C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_segment_sums": (_int, [_vp, _vp, _int, _int, _i64, _PP, _int, _int, _vp, _vp]),
    "rsseg_segment_majority_u8": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _int, _vp]),
    "rsseg_segment_paint": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _vp]),
    "rsseg_segment_features": (_int, [_vp, _vp, _int, _int, _i64, _PP, _int, _int, _vp, _int, _vp]),
    "rsseg_segment_features_plan": (None, [_int, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_segment_adjacency": (_int, [_vp, _vp, _int, _int, _i64, _vp, _PP, _int, _i64, _vp, C.POINTER(_i64)]),
    "rsseg_segment_adjacency_plan": (None, [_int, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_class_moments": (_int, [_vp, _PP, _int, _int, _i64, _vp, _int, _int, _int, _vp, C.POINTER(_int), _int, _vp, C.POINTER(_i64)]),
    "rsseg_class_moments_plan": (None, [_int, _int, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_isodata_sweep": (_int, [_vp, _PP, _int, _int, _i64, _vp, C.POINTER(_int), _int, C.POINTER(C.c_double), _int, C.POINTER(C.c_double), _vp,
                                   _vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "rsseg_isodata_plan": (None, [_int, _int, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_gmm_sweep": (_int, [_vp, _PP, _int, _int, _i64, _vp, C.POINTER(_int), _int, _int, _int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "rsseg_gmm_plan": (None, [_int, _int, _int, _int, C.POINTER(_int), C.POINTER(_int)]),
    "rsseg_lbp_uniform_u8":(_int, [_vp, _vp, _int, _int, _int, C.c_double, _vp]),
    "rsseg_rank_entropy_u8": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_gaussian_blur_u8": (_int, [_vp, _vp, _int, _int, _int, _vp]),
    "rsseg_confusion_counts": (_int, [_vp, _vp, _int, _vp, _int, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
                                      C.POINTER(_i64), _i64]),
    "rsseg_preprocess_u8": (_int, [_vp, _PP, _int, _int, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double), _PP,
                                   C.POINTER(C.c_double)]),
    "rsseg_radiometric": (_int, [_vp, _vp, _int, _i64, C.c_double, C.c_double, _vp]),
    "rsseg_warp_poly": (_int, [_vp, _PP, _int, _int, _int, _int, C.POINTER(C.c_double), C.c_double, C.c_double, _int, C.c_double, _PP, _int,
                               _int, _int, _vp, C.POINTER(_i64)]),
    "rsseg_host_gaussian_kernel_fixed": (_int, [_int, C.POINTER(_int)]),
    "rsseg_host_lzw_encode": (_i64, [_vp, _i64, _vp, _i64]),
    "rsseg_host_lzw_decode": (_i64, [_vp, _i64, _vp, _i64]),
    "rsseg_host_kmeans_draws": (_int, [C.c_uint32, _i64, _int, _int, C.POINTER(_i64), C.POINTER(C.c_double)]),
    "rsseg_host_pca_model": (_int, [C.POINTER(_i64), _i64, _int, _int, _int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
}

_lib = None


def load(path: str = None, missing_ok=()) -> C.CDLL:
    """Loads the shared library and declares every entry point of include/rsseg.h.  The first call decides: `path` names
    another build of the library than LIB_PATH, and `missing_ok` lists entry points that build may lack (they stay
    undeclared); both exist for comparing an older build with this one (profiles/forest_grid_bench.py), the product path
    calls load() and fails loudly on any missing symbol."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C rs-image-segmentation_amd/csrc).  There is no CPU fallback.")
    try:
        # torch-ROCm ships its own HIP runtime: load it FIRST, so that librsseg_hip.so binds to the runtime that owns
        # the process's device state.  (Loaded the other way round — e.g. build() then smoke() in one process — the
        # system libamdhip64 comes up first and hipGetDeviceCount reports "no ROCm-capable device".)
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if name in missing_ok and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
