"""ctypes binding of libcf_mi355x.so (the C ABI declared in include/cf_abi.h).

The product path is the HIP library.  There is no CPU fallback: if the shared
object is missing or fails to load, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CF_MI355X_LIB") or os.path.join(_HERE, "libcf_mi355x.so")   # override: variant builds (tools/)
HOST_LIB_PATH = os.path.join(_HERE, "libcf_host.so")

CF_OK = 0
CF_EINVAL = -1
CF_ERANGE = -4
CF_ESTATE = -5
CF_KNN_SCORE_SUM = 0
CF_KNN_SCORE_MEAN = 1
CF_NMF_OBSERVED = 0
CF_NMF_GRID = 1
CF_NMF_EPS = 1e-16
CF_BPR_TRIES = 8
CF_SVD_MAX_NV = 256
CF_ALS_MAX_D = 64
CF_TOPN_MAX_N = 1024
CF_SIGS_OWN = 0
CF_SIGS_COMPAT = 1
CF_MAX_K = 192
CF_SPILL_MAX_K = 5000
CF_EIGEN_TRIDIAG = 0
CF_EIGEN_JACOBI = 1
CF_GRAPH_DENSE = 0
CF_GRAPH_CSR = 1
CF_FILTER_CHEBY = 0
CF_FILTER_BINOMIAL = 1
CF_SPLIT_LEAVE_K = 0
CF_SPLIT_RATIO = 1
CF_SPLIT_FOLDS = 2
CF_SPLIT_DROPPED = 255
CF_SPLIT_STATS = 8

# name -> (restype, argtypes); the list is the ABI contract checked by tests.
SIGNATURES = {
    "cf_version": (c_int, []),
    "cf_device_count": (c_int, []),
    "cf_create": (c_int, [c_int, POINTER(c_void_p)]),
    "cf_destroy": (None, [c_void_p]),
    "cf_release_workspaces": (c_int, [c_void_p]),
    "cf_last_error": (c_char_p, [c_void_p]),
    "cf_set_jacobi": (c_int, [c_void_p, c_float, c_int]),
    "cf_set_eigen_refine": (c_int, [c_void_p, c_int, c_float, c_float]),
    "cf_set_eigen_split": (c_int, [c_void_p, c_int]),
    "cf_set_eigen_lanes": (c_int, [c_void_p, c_int]),
    "cf_debug_eigen_geometry": (c_int, [c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                        POINTER(c_int)]),
    "cf_set_pred_pack": (c_int, [c_void_p, c_int]),
    "cf_debug_split_schedule": (c_int, [c_int, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "cf_set_step_masks": (c_int, [c_void_p, c_int]),
    "cf_set_local_wlim": (c_int, [c_void_p, c_int]),
    "cf_debug_predict_nmax": (c_int, [c_int]),
    "cf_set_knn2_topk": (c_int, [c_void_p, c_uint32]),
    "cf_set_eigen_method": (c_int, [c_void_p, c_int]),
    "cf_debug_stats": (c_int, [c_void_p, c_int, c_void_p]),
    "cf_eigen_bucket_timing": (c_int, [c_void_p, c_int, c_void_p]),
    "cf_eigen_bucket_timing_split": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "cf_debug_phases": (c_int, [c_void_p, c_int, c_void_p]),
    "cf_debug_spill": (c_int, [c_void_p, c_int, c_void_p]),
    "cf_debug_tri": (c_int, [c_void_p, c_int, c_void_p]),
    "cf_item_graph_upload": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "cf_item_graph_upload_dense": (c_int, [c_void_p, c_uint32, c_void_p, c_int]),
    "cf_item_graph_device": (c_void_p, [c_void_p, POINTER(c_uint32)]),
    "cf_set_graph_layout": (c_int, [c_void_p, c_int]),
    "cf_graph_info": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_item_cosine_edges": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]),
    "cf_plan_create": (c_int, [c_void_p, c_uint32, c_void_p, POINTER(c_void_p)]),
    "cf_plan_destroy": (None, [c_void_p]),
    "cf_evec_slots": (c_uint64, [c_uint32]),
    "cf_evec_offsets": (c_uint64, [c_uint32, c_void_p, c_void_p]),
    "cf_eigen_batch": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "cf_eigen_run": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p]),
    "cf_predict_precomp": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "cf_predict_precomp_sel": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "cf_predict_precomp_multi": (c_int, [c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "cf_predict_precomp_sel_f32": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "cf_predict_precomp_multi_f32": (c_int, [c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_uint64, c_int, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "cf_step_run": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_step_timing": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cf_predict_run_f64": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "cf_predict_run_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "cf_item_cosine": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int,
                               c_void_p]),
    "cf_item_cosine_run": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                   c_int, c_void_p, c_void_p]),
    "cf_knn_regroup": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32] + [c_void_p] * 12 + [c_uint64]),
    "cf_knn_regroup_run": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32] + [c_void_p] * 12 + [c_uint64, c_void_p]),
    "cf_fold_order": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p]),
    "cf_fold_order_run": (c_int, [c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_kcore": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p,
                         POINTER(c_uint32)]),
    "cf_kcore_run": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p,
                             POINTER(c_uint32), c_void_p]),
    "cf_holdout_split": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64,
                                 c_uint32, c_uint32, c_int, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p]),
    "cf_holdout_split_run": (c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64,
                                     c_uint32, c_uint32, c_int, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p,
                                     c_void_p]),
    "cf_split_timing": (c_int, [c_void_p, c_void_p]),
    "cf_prep_timing": (c_int, [c_void_p, c_void_p]),
    "cf_set_knn2_chunk": (c_int, [c_void_p, c_uint32]),
    "cf_knn2_chunks": (c_int, [c_void_p, c_void_p]),
    "cf_knn2_exactness": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cf_knn2_timing": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_knn_predict": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_graph_filter": (c_int, [c_void_p, c_int, c_uint32, ctypes.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_uint32, c_void_p]),
    "cf_graph_filter_timing": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cf_debug_filter_lanes": (c_int, [c_uint32, ctypes.c_uint64]),
    "cf_local_calc": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_cost_split": (c_int, [c_uint32, c_void_p, c_int, c_void_p]),
    "cf_pack_eigen_run": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "cf_eigen_batch_multi": (c_int, [c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_uint64, c_void_p]),
    "cf_als_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_double, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_als_error": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p,
                             c_void_p, c_double, c_double, c_void_p]),
    "cf_als_predict": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p,
                               c_void_p]),
    "cf_sgd_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
    "cf_sgd_timing": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cf_sgd_error": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_void_p]),
    "cf_sgd_predict": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_double, c_int, c_double, c_double, c_void_p]),
    "cf_svdpp_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_uint32, c_void_p]),
    "cf_svdpp_timing": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_svdpp_predict": (c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_double, c_double, c_void_p]),
    "cf_svd_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_uint32, c_uint32, c_uint32, c_double, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_svd_matvec": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_debug_svd_wave_max": (c_int, []),
    "cf_debug_small_svd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_debug_als_segment": (c_int, []),
    "cf_debug_als_low_max": (c_int, []),
    "cf_mf_topn": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                           c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_set_topn_block": (c_int, [c_void_p, c_uint32]),
    "cf_debug_topn_tile_users": (c_int, []),
    "cf_debug_topn_tile_items": (c_int, []),
    "cf_mf_rank_eval": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_double,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p,
                                c_void_p]),
    "cf_debug_rank_targets": (c_int, []),
    "cf_debug_rank_walk": (c_int, []),
    "cf_knn_topn": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                            c_uint32, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_knn_rank_eval": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "cf_debug_knn_topn_walk": (c_int, []),
    "cf_ials_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32] + [c_void_p] * 10 + [c_uint32] + [c_void_p] * 4),
    "cf_ials_loss": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32] + [c_void_p] * 13),
    "cf_mf_gram": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "cf_debug_ials_gram_rows": (c_int, []),
    "cf_nmf_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32] + [c_void_p] * 6 + [c_int, c_uint32] + [c_void_p] * 4),
    "cf_nmf_loss": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32] + [c_void_p] * 6 + [c_int] + [c_void_p] * 3),
    "cf_mf_colsum": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p]),
    "cf_debug_nmf_sum_rows": (c_int, []),
    "cf_bpr_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32] + [c_void_p] * 10),
    "cf_bpr_sample": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p]),
    "cf_bpr_timing": (c_int, [c_void_p, c_void_p]),
    "cf_debug_bpr_tries": (c_int, []),
    "cf_ease_fit": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_double]),
    "cf_ease_gram": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p]),
    "cf_ease_weights": (c_int, [c_void_p, c_void_p, c_void_p]),
    "cf_ease_upload": (c_int, [c_void_p, c_uint32, c_void_p]),
    "cf_ease_topn": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_uint32,
                             c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "cf_ease_rank_eval": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]),
    "cf_ease_timing": (c_int, [c_void_p, c_void_p]),
    "cf_debug_ease_inverse": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_int, c_double,
                                      c_void_p]),
    "cf_debug_ease_block": (c_int, []),
    "cf_debug_ease_cols": (c_int, []),
    "cf_debug_ease_unroll": (c_int, []),
    "cf_eigen_batch_stream": (c_int, [c_void_p, c_int, c_uint32, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p,
                                      c_void_p]),
}


class EigenChunk(ctypes.Structure):
    """cf_eigen_chunk (cf_abi.h): one chunk of cf_eigen_batch_stream's records."""
    _fields_ = [("first", c_uint32), ("count", c_uint32), ("item_off", POINTER(c_uint64)),
                ("m", POINTER(c_int32)), ("sigs", POINTER(c_float)), ("evals", POINTER(c_float)),
                ("packed_off", POINTER(c_uint64)), ("evecs", POINTER(c_float))]


class EigenStreamStats(ctypes.Structure):
    """cf_eigen_stream_stats (cf_abi.h)."""
    _fields_ = [("chunks", c_uint32), ("chunk_slot_bytes", c_uint64), ("max_chunk_slot_bytes", c_uint64),
                ("own_peak_bytes", c_uint64), ("device_peak_bytes", c_uint64)]


class AlsStats(ctypes.Structure):
    """cf_als_stats (cf_abi.h)."""
    _fields_ = [("supersteps", c_uint32), ("updates", c_uint64), ("n_not_pd", c_uint64),
                ("update_ms", c_float), ("scatter_ms", c_float)]


class IalsStats(ctypes.Structure):
    """cf_ials_stats (cf_abi.h)."""
    _fields_ = [("sweeps", c_uint32), ("n_not_pd", c_uint64), ("gram_ms", c_float), ("update_ms", c_float),
                ("loss_ms", c_float)]


class NmfStats(ctypes.Structure):
    """cf_nmf_stats (cf_abi.h)."""
    _fields_ = [("sweeps", c_uint32), ("n_floored", c_uint64), ("sum_ms", c_float), ("update_ms", c_float),
                ("loss_ms", c_float)]


class BprParams(ctypes.Structure):
    """cf_bpr_params (cf_abi.h)."""
    _fields_ = [("lr", c_double), ("reg_user", c_double), ("reg_item", c_double), ("reg_bias", c_double),
                ("seed", c_uint64), ("first_sweep", c_uint32), ("n_sweeps", c_uint32)]


class BprStats(ctypes.Structure):
    """cf_bpr_stats (cf_abi.h)."""
    _fields_ = [("sweeps", c_uint32), ("triples", c_uint64), ("n_skipped", c_uint64), ("n_nan", c_uint64),
                ("sample_ms", c_float), ("reduce_ms", c_float), ("apply_ms", c_float)]


class SgdParams(ctypes.Structure):
    """cf_sgd_params (cf_abi.h)."""
    _fields_ = [("lambda_", c_double), ("gamma", c_double), ("step_dec", c_double), ("tol", c_double),
                ("minval", c_double), ("maxval", c_double), ("global_mean", c_double), ("max_updates", c_uint64),
                ("max_supersteps", c_uint32)]


class SgdStats(ctypes.Structure):
    """cf_sgd_stats (cf_abi.h)."""
    _fields_ = [("supersteps", c_uint32), ("updates", c_uint64), ("messages", c_uint64), ("n_nan", c_uint64),
                ("gamma_next", c_double), ("reduce_ms", c_float), ("apply_ms", c_float)]


class SvdppParams(ctypes.Structure):
    """cf_svdpp_params (cf_abi.h)."""
    _fields_ = [(k, c_float) for k in ("user_bias_step", "user_bias_reg", "item_bias_step", "item_bias_reg",
                                       "user_factor_step", "user_factor_reg", "item_factor_step", "item_factor_reg",
                                       "item_factor2_step", "item_factor2_reg")] + \
               [("step_dec", c_double), ("minval", c_double), ("maxval", c_double), ("global_mean", c_double),
                ("max_updates", c_uint64), ("max_supersteps", c_uint32)]


class SvdppStats(ctypes.Structure):
    """cf_svdpp_stats (cf_abi.h)."""
    _fields_ = [("supersteps", c_uint32), ("updates", c_uint64), ("messages", c_uint64), ("n_nan", c_uint64),
                ("user_bias_step", c_float), ("item_bias_step", c_float), ("user_factor_step", c_float),
                ("item_factor_step", c_float), ("item_factor2_step", c_float), ("reduce_ms", c_float),
                ("apply_ms", c_float)]


class SvdStats(ctypes.Structure):
    """cf_svd_stats (cf_abi.h)."""
    _fields_ = [("nconv", c_uint32), ("passes", c_uint32), ("products", c_uint32), ("matvec_ms", c_float),
                ("ortho_ms", c_float), ("rotate_ms", c_float)]


class TopnStats(ctypes.Structure):
    """cf_topn_stats (cf_abi.h)."""
    _fields_ = [("blocks", c_uint32), ("n_nan", c_uint64), ("score_ms", c_float), ("select_ms", c_float)]


class RankUser(ctypes.Structure):
    """cf_rank_user (cf_abi.h): 64 bytes; api.RANK_USER_DTYPE is the same layout for numpy."""
    _fields_ = [("n_cand", c_uint32), ("n_rel", c_uint32), ("hits", c_uint32), ("reserved", c_uint32),
                ("precision", c_double), ("recall", c_double), ("ndcg", c_double), ("ap", c_double),
                ("rr", c_double), ("auc", c_double)]


class RankSummary(ctypes.Structure):
    """cf_rank_summary (cf_abi.h)."""
    _fields_ = [("users_evaluated", c_uint32), ("users_auc", c_uint32), ("edges_counted", c_uint64),
                ("edges_skipped", c_uint64), ("n_nan_held", c_uint64), ("precision", c_double), ("recall", c_double),
                ("ndcg", c_double), ("map", c_double), ("mrr", c_double), ("auc", c_double), ("mpr", c_double),
                ("blocks", c_uint32), ("score_ms", c_float), ("rank_ms", c_float)]


EIGEN_SINK =ctypes.CFUNCTYPE(c_int, c_void_p, POINTER(EigenChunk))

_lib = None


class NativeError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libcf_mi355x.so (raises NativeError if it is missing: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} not built; run `make` or __graft_entry__.build()")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("CF_MI355X_LIB"):   # an older variant build (A/B runs): skip
                continue
            raise NativeError(f"{LIB_PATH} does not export {name}")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a) -> c_void_p:
    """Raw pointer of a numpy array or a torch tensor (device pointers pass through)."""
    if a is None:
        return c_void_p(0)
    if hasattr(a, "data_ptr"):
        return c_void_p(a.data_ptr())
    return c_void_p(a.ctypes.data)
