"""ctypes binding of libcarskit_mi355x.so (include/carskit_mi355x.h).

This is the only way Python reaches the compute path; there is no Python or CPU fallback.  If the
shared library is missing (not built) loading raises; without a HIP device cmi_create fails with
CMI_E_NO_DEVICE and `Instance(...)` raises `CmiError`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMI_LIB_PATH") or os.path.join(_HERE, "lib", "libcarskit_mi355x.so")   # CMI_LIB_PATH: experiments with variant builds

OK, E_INVALID, E_NO_DEVICE, E_HIP, E_NUMERIC, E_UNSUPPORTED, E_HOST, E_BUSY = 0, -1, -2, -3, -4, -5, -6, -7

MODEL_IDS = {"BiasedMF": 0, "CAMF_C": 1, "CAMF_CI": 2, "CAMF_CU": 3, "CAMF_CUCI": 4, "PMF": 5,
             "SVD++": 6, "CAMF_ICS": 7, "CAMF_LCS": 8, "CAMF_MCS": 9}
STATE_IDS = {"P": 0, "Q": 1, "userBias": 2, "itemBias": 3, "condBias": 4, "ucBias": 5, "icBias": 6,
             "Y": 7, "ccMatrix": 8, "cfMatrix": 9, "cVector": 10}
MODEL_STATES = {
    "BiasedMF": ("P", "Q", "userBias", "itemBias"),
    "CAMF_C": ("P", "Q", "userBias", "itemBias", "condBias"),
    "CAMF_CI": ("P", "Q", "userBias", "icBias"),
    "CAMF_CU": ("P", "Q", "itemBias", "ucBias"),
    "CAMF_CUCI": ("P", "Q", "ucBias", "icBias"),
    "PMF": ("P", "Q"),
    "SVD++": ("P", "Q", "userBias", "itemBias", "Y"),
    "CAMF_ICS": ("P", "Q", "ccMatrix"),
    "CAMF_LCS": ("P", "Q", "cfMatrix"),
    "CAMF_MCS": ("P", "Q", "cVector"),
}
# the state keyed by item (replicated and reconciled across GPUs when tuples are sharded by user)
ITEM_SIDE = {"Q", "itemBias", "icBias", "condBias"}

FLAG_STATE_F64 = 0x1
FLAG_SCHED_SERIAL = 0x2
FLAG_STRICT = 0x4
FLAG_NO_GRAPH = 0x10
FLAG_SCHED_CHAIN = 0x80
FLAG_NO_CHAIN = 0x100
FLAG_SCHED_OWNER = 0x200
FLAG_NO_OWNER = 0x400
FLAG_SPOKE_ARENA = 0x800
FLAG_NO_ARENA = 0x1000
FM_FLAG_DETERMINISTIC = 0x1      # round-5 name of what is now the default (accepted, no effect)
FM_FLAG_RELAXED_SUMS = 0x2       # opt into the LDS-atomic sums (faster, last bits vary run to run)
OWN_HUB_FWD, OWN_HUB_LATE, OWN_HUB_STORE, OWN_SPK_FWD, OWN_SPK_STORE = 1, 2, 4, 8, 16

# every symbol include/carskit_mi355x.h declares: (name, restype, argtypes)
_vp, _i64, _i32, _dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
SYMBOLS = [
    ("cmi_abi_version", C.c_int, []),
    ("cmi_device_count", C.c_int, []),
    ("cmi_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_destroy", C.c_int, [_vp]),
    ("cmi_last_error", C.c_char_p, [_vp]),
    ("cmi_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    ("cmi_set_state", C.c_int, [_vp, C.c_int, _vp, _i64, C.c_int]),
    ("cmi_get_state", C.c_int, [_vp, C.c_int, _vp, _i64, C.c_int]),
    ("cmi_set_sim_params", C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int]),
    ("cmi_set_hparams", C.c_int, [_vp, _dbl, _dbl, _dbl, _dbl, _dbl]),
    ("cmi_set_device_share", C.c_int, [_vp, C.c_int]),
    ("cmi_train_epoch", C.c_int, [_vp, _dbl, C.POINTER(_dbl)]),
    ("cmi_train", C.c_int, [_vp, C.c_int, _dbl, _dbl, C.c_int, _dbl, C.c_int, _vp, _vp, C.POINTER(C.c_int),
                            C.POINTER(_dbl)]),
    ("cmi_train_from", C.c_int, [_vp, C.c_int, _dbl, C.c_int, _dbl, _dbl, C.c_int, _dbl, C.c_int, _vp, _vp, C.POINTER(C.c_int),
                                 C.POINTER(_dbl)]),
    ("cmi_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_eval_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _dbl, _dbl, _vp, C.POINTER(_i64)]),
    ("cmi_set_eval_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    ("cmi_eval_resident", C.c_int, [_vp, _dbl, _dbl, _vp, C.POINTER(_i64)]),
    ("cmi_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                    C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_fm_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                       C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_last_rank_ms", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(_dbl)]),
    ("cmi_last_rank_host_ms", C.c_int, [_vp, _vp]),
    ("cmi_last_rank_kernel_ms", C.c_int, [_vp, _vp]),
    ("cmi_group_set_eval_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    ("cmi_group_eval_resident", C.c_int, [_vp, _dbl, _dbl, _vp, C.POINTER(_i64)]),
    ("cmi_comm_unique_id", C.c_int, [_vp]),
    ("cmi_comm_init", C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    ("cmi_comm_exchange", C.c_int, [_vp, _dbl]),
    ("cmi_comm_train_epoch", C.c_int, [_vp, _dbl, _dbl, C.POINTER(_dbl)]),
    ("cmi_comm_last_exchange_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_rank_plan", C.c_int, [C.c_int32, C.c_int32, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int,
                                C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("cmi_rank_list_measures", C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("cmi_narrow_runs", C.c_int, [_i64, _vp, _i64, _i64, _vp, C.POINTER(_i64)]),
    ("cmi_conflict_free_blocks", C.c_int, [_i64, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, _i64, C.POINTER(_i64)]),
    ("cmi_svdpp_team_rows", C.c_int, [C.c_int, C.c_int, C.POINTER(_i64)]),
    ("cmi_java_int_hashset_order", C.c_int, [_i64, _vp, _vp, C.POINTER(_i64)]),
    ("cmi_state_device_ptr", C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(C.c_int)]),
    ("cmi_stream", C.c_int, [_vp, C.POINTER(_vp)]),
    ("cmi_synchronize", C.c_int, [_vp]),
    ("cmi_train_epoch_async", C.c_int, [_vp, _dbl]),
    ("cmi_last_loss", C.c_int, [_vp, C.POINTER(_dbl)]),
    ("cmi_save_model", C.c_int, [_vp, C.c_char_p, C.c_double, C.c_double, C.c_int]),
    ("cmi_load_model", C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("cmi_measure_hbm", C.c_int, [C.c_int, _i64, C.POINTER(C.c_double)]),
    ("cmi_schedule_info", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_schedule_traffic", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_schedule_note", C.c_char_p, [_vp]),
    ("cmi_arena_positions", C.c_int, [_i64, _vp, _i32, _vp, _vp]),
    ("cmi_exchange_setup", C.c_int, [_vp, _i64, C.POINTER(_vp), C.POINTER(_i64)]),
    ("cmi_group_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_uint, C.POINTER(_vp)]),
    ("cmi_group_destroy", C.c_int, [_vp]),
    ("cmi_group_last_error", C.c_char_p, [_vp]),
    ("cmi_group_size", C.c_int, [_vp]),
    ("cmi_group_set_hparams", C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    ("cmi_group_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    ("cmi_group_set_state", C.c_int, [_vp, C.c_int, _vp, _i64, C.c_int]),
    ("cmi_group_get_state", C.c_int, [_vp, C.c_int, _vp, _i64, C.c_int]),
    ("cmi_group_train_epoch", C.c_int, [_vp, C.c_double, C.POINTER(C.c_double)]),
    ("cmi_group_set_lr_scale", C.c_int, [_vp, C.c_double]),
    ("cmi_group_train", C.c_int, [_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, _vp, _vp, C.POINTER(C.c_int),
                                  C.POINTER(C.c_double)]),
    ("cmi_group_train_from", C.c_int, [_vp, C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, _vp, _vp,
                                       C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("cmi_group_eval_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, C.POINTER(_i64)]),
    ("cmi_group_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, _vp]),
    ("cmi_group_shard_info", C.c_int, [_vp, C.c_int, C.POINTER(_i64)]),
    ("cmi_group_last_times", C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("cmi_group_exchange_path", C.c_char_p, [_vp]),
    ("cmi_group_member", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("cmi_exchange_pack", C.c_int, [_vp]),
    ("cmi_exchange_apply", C.c_int, [_vp, C.c_double]),
    ("cmi_loss_device_ptr", C.c_int, [_vp, C.POINTER(_vp)]),
    ("cmi_last_epoch_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_level_schedule", C.c_int, [_i64, _vp, _vp, _i32, _i32, C.c_int, _vp, _vp, _i64, C.POINTER(_i64)]),
    ("cmi_owner_schedule", C.c_int, [_i64, _vp, _vp, _i32, _i32, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.POINTER(C.c_int)]),
    ("cmi_chain_schedule", C.c_int, [_i64, _vp, _vp, _i32, _i32, C.c_int, C.c_int, _vp, _vp, _i64, _vp, _i64, C.POINTER(_i64),
                                     C.POINTER(_i64), C.POINTER(C.c_int)]),
    ("cmi_chain_schedule_device", C.c_int, [C.c_int, _i64, _vp, _vp, _i32, _i32, C.c_int, C.c_int, _vp, _vp, _i64, _vp, _i64, C.POINTER(_i64),
                                     C.POINTER(_i64), C.POINTER(C.c_int)]),
    ("cmi_dao_read", C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    ("cmi_dao_read_shared", C.c_int, [C.c_char_p, _vp, C.POINTER(_vp)]),
    ("cmi_dao_destroy", C.c_int, [_vp]),
    ("cmi_dao_last_error", C.c_char_p, [_vp]),
    ("cmi_dao_counts", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_dao_matrix", C.c_int, [_vp, _vp, _vp, _vp]),
    ("cmi_dao_ui_maps", C.c_int, [_vp, _vp, _vp]),
    ("cmi_dao_ctx_nnz", _i64, [_vp]),
    ("cmi_dao_ctx_table", C.c_int, [_vp, _vp, _vp]),
    ("cmi_dao_cond_info", C.c_int, [_vp, _vp, _vp, C.POINTER(_i32)]),
    ("cmi_dao_rating_scale", C.c_int, [_vp, _vp, _i32, C.POINTER(_i32)]),
    ("cmi_dao_raw_id", C.c_char_p, [_vp, C.c_int, _i32]),
    ("cmi_java_hashmap_order", C.c_int, [_i64, _vp, _vp, C.POINTER(C.c_int)]),
    ("cmi_transform_compact_to_binary", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]),
    ("cmi_validate_data_format", C.c_int, [C.c_char_p]),
    ("cmi_transform", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]),
    ("cmi_fm_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_fm_destroy", C.c_int, [_vp]),
    ("cmi_fm_last_error", C.c_char_p, [_vp]),
    ("cmi_fm_set_hparams", C.c_int, [_vp, _dbl, _dbl, _i64]),
    ("cmi_fm_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp]),
    ("cmi_fm_set_model", C.c_int, [_vp, _dbl, _vp, _vp]),
    ("cmi_fm_get_model", C.c_int, [_vp, C.POINTER(_dbl), _vp, _vp]),
    ("cmi_fm_init", C.c_int, [_vp]),
    ("cmi_fm_sweep", C.c_int, [_vp]),
    ("cmi_fm_train", C.c_int, [_vp, C.c_int]),
    ("cmi_fm_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_knn_measure", C.c_int, [C.c_char_p]),
    ("cmi_knn_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_knn_destroy", C.c_int, [_vp]),
    ("cmi_knn_last_error", C.c_char_p, [_vp]),
    ("cmi_knn_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_knn_build", C.c_int, [_vp, C.c_int, C.c_int, _dbl, _dbl]),
    ("cmi_knn_get_similarity", C.c_int, [_vp, C.c_int32, C.c_int32, _vp]),
    ("cmi_knn_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, C.c_int, _dbl, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_knn_last_build_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_knn_ranking_batch", C.c_int, [_vp, _i64, _vp, _vp, C.c_int, _dbl, _vp]),
    ("cmi_knn_eval_rankings", C.c_int, [_vp, C.c_int, _dbl, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                        C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_knn_last_rank_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_slope_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_slope_destroy", C.c_int, [_vp]),
    ("cmi_slope_last_error", C.c_char_p, [_vp]),
    ("cmi_slope_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_slope_build", C.c_int, [_vp]),
    ("cmi_slope_get_deviation", C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    ("cmi_slope_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _dbl, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_slope_last_build_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_slope_eval_rankings", C.c_int, [_vp, _dbl, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                          C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_slope_last_rank_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_nmf_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_nmf_destroy", C.c_int, [_vp]),
    ("cmi_nmf_last_error", C.c_char_p, [_vp]),
    ("cmi_nmf_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_nmf_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_nmf_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_nmf_iterate", C.c_int, [_vp, C.POINTER(_dbl)]),
    ("cmi_nmf_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_nmf_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_topn_nmf_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                        C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_topn_nmf_last_rank_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_slim_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_slim_destroy", C.c_int, [_vp]),
    ("cmi_slim_last_error", C.c_char_p, [_vp]),
    ("cmi_slim_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_slim_build_neighbors", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dbl, _dbl]),
    ("cmi_slim_cut_neighbors", C.c_int, [C.c_int32, _vp, C.c_int, _vp, C.POINTER(C.c_int32)]),
    ("cmi_slim_get_neighbors", C.c_int, [_vp, _vp, _vp]),
    ("cmi_slim_set_weights", C.c_int, [_vp, _vp]),
    ("cmi_slim_get_weights", C.c_int, [_vp, _vp]),
    ("cmi_slim_iterate", C.c_int, [_vp, _dbl, _dbl, C.POINTER(_dbl)]),
    ("cmi_slim_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_slim_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                         C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_slim_last_build_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_slim_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_rankals_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_rankals_destroy", C.c_int, [_vp]),
    ("cmi_rankals_last_error", C.c_char_p, [_vp]),
    ("cmi_rankals_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_rankals_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_rankals_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_rankals_iterate", C.c_int, [_vp, C.c_int]),
    ("cmi_rankals_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_rankals_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                            C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_rankals_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_rankals_invert", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    ("cmi_bpr_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_bpr_destroy", C.c_int, [_vp]),
    ("cmi_bpr_last_error", C.c_char_p, [_vp]),
    ("cmi_bpr_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_bpr_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_bpr_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_bpr_set_random_state", C.c_int, [_vp, _i64]),
    ("cmi_bpr_get_random_state", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_bpr_sample", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("cmi_bpr_iterate", C.c_int, [_vp, _dbl, _dbl, _dbl, C.POINTER(_dbl)]),
    ("cmi_bpr_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_bpr_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                        C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_bpr_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_bpr_last_schedule", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_bpr_levels", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i64)]),
    ("cmi_bpr_sample_host", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, C.POINTER(_i64), _i64, _vp, _vp, _vp]),
    ("cmi_bpr_rank_block", C.c_int, []),
    ("cmi_java_next_ints", C.c_int, [C.POINTER(_i64), _i32, _i64, _vp, C.c_int]),
    ("cmi_java_exp_log", C.c_int, [_i64, _vp, _vp, _vp, C.c_int]),
    ("cmi_lrmf_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_lrmf_destroy", C.c_int, [_vp]),
    ("cmi_lrmf_last_error", C.c_char_p, [_vp]),
    ("cmi_lrmf_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_lrmf_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_lrmf_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_lrmf_iterate", C.c_int, [_vp, _dbl, _dbl, _dbl, C.POINTER(_dbl)]),
    ("cmi_lrmf_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_lrmf_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                         C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_lrmf_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_lrmf_last_schedule", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_lrmf_levels", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i32), C.POINTER(_i64)]),
    ("cmi_lrmf_lds_rows", C.c_int, [C.c_int]),
    ("cmi_lrmf_block", C.c_int, []),
    ("cmi_ranksgd_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_ranksgd_destroy", C.c_int, [_vp]),
    ("cmi_ranksgd_last_error", C.c_char_p, [_vp]),
    ("cmi_ranksgd_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_ranksgd_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_ranksgd_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_ranksgd_set_random_state", C.c_int, [_vp, _i64]),
    ("cmi_ranksgd_get_random_state", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_ranksgd_sample", C.c_int, [_vp, C.c_int, _i64, _vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("cmi_ranksgd_iterate", C.c_int, [_vp, _dbl, C.POINTER(_dbl)]),
    ("cmi_ranksgd_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_ranksgd_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                            C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_ranksgd_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_ranksgd_last_schedule", C.c_int, [_vp, C.POINTER(_i64)]),
    ("cmi_ranksgd_item_table", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, C.c_uint, _vp, _vp, C.POINTER(_i32)]),
    ("cmi_ranksgd_tries", C.c_int, [_i64, _i32, _vp, _vp, _i64, _vp, C.c_int]),
    ("cmi_ranksgd_assign_host", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, _i64, _vp, _vp, C.POINTER(_i64)]),
    ("cmi_ranksgd_sample_host", C.c_int, [C.c_int, C.c_int, _i64, _vp, _vp, _vp, C.c_uint, C.POINTER(_i64), _vp, _vp, _vp, _vp,
                                          C.POINTER(_i64), C.POINTER(_i64)]),
    ("cmi_cptf_create", C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_cptf_destroy", C.c_int, [_vp]),
    ("cmi_cptf_last_error", C.c_char_p, [_vp]),
    ("cmi_cptf_set_entries", C.c_int, [_vp, _i64, _vp, _vp]),
    ("cmi_cptf_set_context_keys", C.c_int, [_vp, _i32, _vp]),
    ("cmi_cptf_set_rating_range", C.c_int, [_vp, _dbl, _dbl]),
    ("cmi_cptf_set_model", C.c_int, [_vp, _vp]),
    ("cmi_cptf_get_model", C.c_int, [_vp, _vp]),
    ("cmi_cptf_iterate", C.c_int, [_vp, _dbl, _dbl, C.POINTER(_dbl)]),
    ("cmi_cptf_predict_batch", C.c_int, [_vp, _i64, _vp, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_cptf_eval_rankings", C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _dbl, C.c_int, C.c_int,
                                         C.c_int, _vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp]),
    ("cmi_cptf_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_cptf_ctx_in_lds", C.c_int, [_vp]),
    ("cmi_cptf_tensor_build", C.c_int, [_i64, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i64, _vp, C.c_uint,
                                        C.POINTER(_i32), _vp, _vp, _vp, _vp, _vp, C.POINTER(_i64), _vp, _vp, C.POINTER(_i64), _vp, _vp,
                                        _vp]),
    ("cmi_bpmf_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(_vp)]),
    ("cmi_bpmf_destroy", C.c_int, [_vp]),
    ("cmi_bpmf_last_error", C.c_char_p, [_vp]),
    ("cmi_bpmf_set_ratings", C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    ("cmi_bpmf_set_global_mean", C.c_int, [_vp, _dbl]),
    ("cmi_bpmf_get_global_mean", C.c_int, [_vp, C.POINTER(_dbl)]),
    ("cmi_bpmf_set_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_bpmf_get_model", C.c_int, [_vp, _vp, _vp]),
    ("cmi_bpmf_set_stream", C.c_int, [_vp, _i64, C.c_int, _dbl]),
    ("cmi_bpmf_get_stream", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(_dbl)]),
    ("cmi_bpmf_init_hyper", C.c_int, [_vp]),
    ("cmi_bpmf_get_hyper", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("cmi_bpmf_set_hyper", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("cmi_bpmf_iterate", C.c_int, [_vp, C.POINTER(_dbl)]),
    ("cmi_bpmf_last_iter_ms", C.c_int, [_vp, C.POINTER(C.c_float)]),
    ("cmi_bpmf_predict_batch", C.c_int, [_vp, _i64, _vp, _vp, C.c_int, _dbl, _dbl, _vp]),
    ("cmi_bpmf_sample_side", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.POINTER(_i64)]),
    ("cmi_java_next_gaussians", C.c_int, [C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(_dbl), _i64, _vp]),
    ("cmi_bpmf_gauss_attempts", _i64, [_i64]),
    ("cmi_bpmf_moments", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int]),
    ("cmi_bpmf_hyper_host", C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(C.c_int), C.POINTER(_dbl)]),
    ("cmi_fm_synchronize", C.c_int, [_vp]),
    ("cmi_fm_stream", C.c_int, [_vp, C.POINTER(_vp)]),
    ("cmi_fm_num_phases", C.c_int, [_vp]),
    ("cmi_fm_phase_reduce", C.c_int, [_vp, C.c_int]),
    ("cmi_fm_phase_buffer", C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_i64)]),
    ("cmi_fm_phase_apply", C.c_int, [_vp, C.c_int]),
    ("cmi_fm_phase_run", C.c_int, [_vp, C.c_int]),
    ("cmi_fm_layout", C.c_int, [_vp, _vp]),
    ("cmi_fm_comm_init", C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    ("cmi_fm_comm_sweep", C.c_int, [_vp]),
    ("cmi_fm_time_reduce", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_dbl)]),
]

_LIB = None


RANK_MEASURES = ("Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN", "MAP5", "MAP10", "MAPN",
                 "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10", "MRRN", "D5", "D10", "DN")


def java_int_hashset_order(values):
    v = np.ascontiguousarray(values, dtype=np.int32)
    out, n = np.zeros(max(len(v), 1), np.int32), _i64()
    rc = lib().cmi_java_int_hashset_order(len(v), _p(v), _p(out), C.byref(n))
    if rc:
        raise CmiError(rc, "cmi_java_int_hashset_order")
    return out[:n.value].copy()


def narrow_runs(level_off, max_tuples=256, min_levels=16):
    off = np.ascontiguousarray(level_off, dtype=np.int64)
    run = np.zeros(max(len(off) - 1, 1), np.int32)
    nl = _i64()
    rc = lib().cmi_narrow_runs(len(off) - 1, _p(off), max_tuples, min_levels, _p(run), C.byref(nl))
    if rc:
        raise CmiError(rc, "cmi_narrow_runs")
    return run[:len(off) - 1].copy(), nl.value


def conflict_free_blocks(u, j, n_users, n_items, max_block=64):
    u = np.ascontiguousarray(u, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    nb = _i64()
    rc = lib().cmi_conflict_free_blocks(len(u), _p(u), _p(j), n_users, n_items, max_block, None, 0, C.byref(nb))
    if rc:
        raise CmiError(rc, "cmi_conflict_free_blocks")
    off = np.zeros(nb.value + 1, np.int32)
    rc = lib().cmi_conflict_free_blocks(len(u), _p(u), _p(j), n_users, n_items, max_block, _p(off), len(off), C.byref(nb))
    if rc:
        raise CmiError(rc, "cmi_conflict_free_blocks")
    return off


def svdpp_team_rows(k, f64):
    """Host-only: the most rated items of a user whose Y rows the SVD++ team kernel keeps in LDS at k factors (0: k out of range)"""
    return int(lib().cmi_svdpp_team_rows(int(k), 1 if f64 else 0, None))


def svdpp_team_lds(k, f64):
    """Host-only: the dynamic LDS bytes of the SVD++ team kernel's launch at k factors"""
    n = _i64()
    lib().cmi_svdpp_team_rows(int(k), 1 if f64 else 0, C.byref(n))
    return n.value


def rank_list_measures(ranked, truth, num_dropped, num_recs):
    """Host-only: {measure: value} of one ranked list (already cut at num_recs), as cmi_eval_rankings computes per query."""
    rk = np.ascontiguousarray(ranked, dtype=np.int32)
    tr = np.ascontiguousarray(sorted(set(truth)), dtype=np.int32)
    out = np.zeros(18)
    rc = lib().cmi_rank_list_measures(_p(rk), len(rk), _p(tr), len(tr), int(num_dropped), int(num_recs), _p(out))
    if rc:
        raise CmiError(rc, "cmi_rank_list_measures")
    return dict(zip(RANK_MEASURES[:18], out.tolist()))


def rank_plan(n_users, n_items, train, test, bin_thold=-1.0, num_ignore=0):
    """Host-only: (candidates, [(user, ctx, correct items, excluded candidate positions), ...]) as cmi_eval_rankings sees them."""
    c32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    tu, tj, tc, tr = c32(train[0]), c32(train[1]), c32(train[2]), f64(train[3])
    su, sj, sc, sr = c32(test[0]), c32(test[1]), c32(test[2]), f64(test[3])
    sizes = (_i64 * 4)()
    args = (n_users, n_items, len(tu), _p(tu), _p(tj), _p(tc), _p(tr), len(su), _p(su), _p(sj), _p(sc), _p(sr), float(bin_thold),
            int(num_ignore), sizes)
    rc = lib().cmi_rank_plan(*args, None, None, None, None, None, None, None)
    if rc:
        raise CmiError(rc, "cmi_rank_plan")
    nc, nq, nt, ne = list(sizes)
    cand, qu, qc = np.zeros(max(nc, 1), np.int32), np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32)
    tp, ti = np.zeros(nq + 1, np.int64), np.zeros(max(nt, 1), np.int32)
    ep, ei = np.zeros(nq + 1, np.int64), np.zeros(max(ne, 1), np.int32)
    rc = lib().cmi_rank_plan(*args, _p(cand), _p(qu), _p(qc), _p(tp), _p(ti), _p(ep), _p(ei))
    if rc:
        raise CmiError(rc, "cmi_rank_plan")
    queries = [(int(qu[q]), int(qc[q]), ti[tp[q]:tp[q + 1]].tolist(), ei[ep[q]:ep[q + 1]].tolist()) for q in range(nq)]
    return cand[:nc].tolist(), queries


COMM_ID_BYTES = 128


def comm_unique_id():
    """cmi_comm_unique_id: the RCCL unique id (bytes) rank 0 creates for a one-process-per-GPU job."""
    buf = (C.c_char * COMM_ID_BYTES)()
    rc = lib().cmi_comm_unique_id(buf)
    if rc:
        raise CmiError(rc, "cmi_comm_unique_id")
    return bytes(buf)


class CmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libcarskit_mi355x error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load the C-ABI library (raises OSError if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not found: build it with `python __graft_entry__.py` or `make -C carskit_amd/csrc` "
                          "(there is no Python/CPU fallback for the compute path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def device_count():
    return lib().cmi_device_count()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _tuples(u, j, ctx, r=None):
    """(u, j, ctx[, r]) as the C ABI takes them: contiguous int32 ids (ctx may be None), float64 ratings"""
    ids = (_c32(u), _c32(j), _c32(ctx))
    return ids if r is None else ids + (np.ascontiguousarray(r, dtype=np.float64),)


def _measures(out, cnt):
    res = dict(zip(("MAE", "RMSE", "NMAE", "rMAE", "rRMSE"), out.tolist()))
    res["n"] = cnt.value
    return res


def measure_hbm(device=0, nbytes=4 << 30):
    """(copy GB/s, random-512-B-row read-modify-write GB/s) measured on the device right now (cmi_measure_hbm)."""
    out = (C.c_double * 2)()
    rc = lib().cmi_measure_hbm(device, nbytes, out)
    if rc != OK:
        raise CmiError(rc, "cmi_measure_hbm")
    return float(out[0]), float(out[1])


def level_schedule(u, j, n_users, n_items, order=0):
    """Host-only: (perm, level_off) of the dependency-level schedule (see cmi_level_schedule)."""
    u = np.ascontiguousarray(u, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    n = len(u)
    nl = _i64()
    rc = lib().cmi_level_schedule(n, _p(u), _p(j), n_users, n_items, order, None, None, 0, C.byref(nl))
    if rc != OK:
        raise CmiError(rc, "cmi_level_schedule")
    perm = np.empty(n, dtype=np.int32)
    off = np.empty(nl.value + 1, dtype=np.int64)
    rc = lib().cmi_level_schedule(n, _p(u), _p(j), n_users, n_items, order, _p(perm), _p(off), len(off), C.byref(nl))
    if rc != OK:
        raise CmiError(rc, "cmi_level_schedule")
    return perm, off


def chain_schedule(u, j, n_users, n_items, hub=-1, max_chain=16):
    """Host-only: (perm, unit_off, level_off, hub_is_item) of the hub-chain level schedule (see cmi_chain_schedule)."""
    u = np.ascontiguousarray(u, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    n = len(u)
    nu, nl, hub_used = _i64(), _i64(), C.c_int()
    rc = lib().cmi_chain_schedule(n, _p(u), _p(j), n_users, n_items, hub, max_chain, None, None, 0, None, 0, C.byref(nu),
                                  C.byref(nl), C.byref(hub_used))
    if rc != OK:
        raise CmiError(rc, "cmi_chain_schedule")
    perm = np.empty(n, dtype=np.int32)
    unit_off = np.empty(nu.value + 1, dtype=np.int32)
    level_off = np.empty(nl.value + 1, dtype=np.int64)
    rc = lib().cmi_chain_schedule(n, _p(u), _p(j), n_users, n_items, hub, max_chain, _p(perm), _p(unit_off), len(unit_off),
                                  _p(level_off), len(level_off), C.byref(nu), C.byref(nl), C.byref(hub_used))
    if rc != OK:
        raise CmiError(rc, "cmi_chain_schedule")
    return perm, unit_off, level_off, bool(hub_used.value)


def chain_schedule_device(u, j, n_users, n_items, hub=-1, max_chain=16, device=0):
    """The same schedule built on the device (cmi_chain_schedule_device; what cmi_set_ratings uses for large sets)."""
    u = np.ascontiguousarray(u, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    n = len(u)
    # (the device build has no count-only form: sized by the host's counts)
    nu, nl, hub_used = _i64(), _i64(), C.c_int()
    rc = lib().cmi_chain_schedule(n, _p(u), _p(j), n_users, n_items, hub, max_chain, None, None, 0, None, 0, C.byref(nu), C.byref(nl), C.byref(hub_used))
    if rc != OK:
        raise CmiError(rc, "cmi_chain_schedule")
    perm = np.empty(n, dtype=np.int32)
    unit_off = np.empty(nu.value + 1, dtype=np.int32)
    level_off = np.empty(nl.value + 1, dtype=np.int64)
    rc = lib().cmi_chain_schedule_device(device, n, _p(u), _p(j), n_users, n_items, hub, max_chain, _p(perm), _p(unit_off), len(unit_off),
                                         _p(level_off), len(level_off), C.byref(nu), C.byref(nl), C.byref(hub_used))
    if rc != OK:
        raise CmiError(rc, "cmi_chain_schedule_device")
    return perm, unit_off[:nu.value + 1], level_off[:nl.value + 1], bool(hub_used.value)


def owner_schedule(u, j, n_users, n_items, n_owners, hub=-1, depth=8):
    """Host-only: (perm, own_off, want, flags, hub_is_item) of the owner (dataflow) schedule (see cmi_owner_schedule)."""
    u = np.ascontiguousarray(u, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    n = len(u)
    perm = np.empty(n, dtype=np.int32)
    own_off = np.empty(n_owners + 1, dtype=np.int64)
    want = np.empty(n, dtype=np.uint32)
    flags = np.empty(n, dtype=np.uint32)
    hub_used = C.c_int()
    rc = lib().cmi_owner_schedule(n, _p(u), _p(j), n_users, n_items, hub, n_owners, depth, _p(perm), _p(own_off), _p(want), _p(flags),
                                  C.byref(hub_used))
    if rc != OK:
        raise CmiError(rc, "cmi_owner_schedule")
    return perm, own_off, want, flags, bool(hub_used.value)


def arena_positions(spoke, n_spokes):
    """Host-only: (next, first) of the spoke arena for a stream of spoke row ids (see cmi_arena_positions)."""
    spoke = np.ascontiguousarray(spoke, dtype=np.int32)
    nxt, first = np.empty(len(spoke), dtype=np.int32), np.empty(n_spokes, dtype=np.int32)
    rc = lib().cmi_arena_positions(len(spoke), _p(spoke), n_spokes, _p(nxt), _p(first))
    if rc != OK:
        raise CmiError(rc, "cmi_arena_positions")
    return nxt, first


def _eval_rankings(fn, chk, h, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
    """Recommender.evalRankings (Recommender.java:668-964).  train/test: (u, j, ctx, r) array tuples.
    Returns {measure: value}; with_lists also returns {(u, ctx): [(item, score), ...]}."""
    c32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    tu, tj, tc, tr = c32(train[0]), c32(train[1]), c32(train[2]), f64(train[3])
    su, sj, sc, sr = c32(test[0]), c32(test[1]), c32(test[2]), f64(test[3])
    out, nq = np.zeros(len(RANK_MEASURES)), _i64()
    n = max(len(su), 1)
    if with_lists:
        qu, qc, qn = (np.zeros(n, np.int32) for _ in range(3))
        items, scores = np.zeros(n * num_recs, np.int32), np.zeros(n * num_recs)
    else:
        qu = qc = qn = items = scores = None
    chk(fn(h, len(tu), _p(tu), _p(tj), _p(tc), _p(tr), len(su), _p(su), _p(sj), _p(sc),
                                       _p(sr), float(bin_thold), int(num_recs), int(num_ignore),
                                       {"ucu": 0, "uc": 1}[strategy], _p(out), C.byref(nq), _p(qu), _p(qc), _p(qn),
                                       _p(items), _p(scores)))
    res = dict(zip(RANK_MEASURES, out.tolist()))
    res["n_queries"] = nq.value
    if not with_lists:
        return res
    lists = {}
    for q in range(nq.value):
        if qn[q] > 0:
            lists[(int(qu[q]), int(qc[q]))] = [(int(items[q * num_recs + i]), float(scores[q * num_recs + i]))
                                               for i in range(qn[q])]
    return res, lists


class _Handle:
    """The lifetime of one C handle: `_api` names its create, destroy and last-error functions; the subclass's __init__ hands the
    create arguments (all but the trailing out-pointer) to this one."""

    _api = ("", "", "")

    def __init__(self, *args):
        self.L = lib()
        create, _, last_error = (getattr(self.L, n) for n in self._api)
        self.h = _vp()
        rc = create(*args, C.byref(self.h))
        if rc != OK:
            self.h = None
            raise CmiError(rc, last_error(None).decode())

    def _chk(self, rc):
        if rc != OK:
            raise CmiError(rc, getattr(self.L, self._api[2])(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._api[1])(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Group(_Handle):
    """One recommender trained over several GPUs from this one process (a `cmi_group_handle`): ratings sharded by user, item-side
    containers merged (mean of the shards' moves) after every epoch through RCCL, or in-process when shards share a device."""

    _api = ("cmi_group_create", "cmi_group_destroy", "cmi_group_last_error")

    def __init__(self, model, k, n_users, n_items, n_conds, n_shards, devices=None, flags=0):
        self.model = model if isinstance(model, str) else {v: n for n, v in MODEL_IDS.items()}[model]
        self.k, self.n_users, self.n_items, self.n_conds, self.num_f = k, n_users, n_items, n_conds, 0
        dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        super().__init__(MODEL_IDS[self.model], k, n_users, n_items, n_conds, n_shards, _p(dev), flags)

    def size(self):
        return self.L.cmi_group_size(self.h)

    def set_hparams(self, regU, regI, regB, regC, global_mean):
        self._chk(self.L.cmi_group_set_hparams(self.h, regU, regI, regB, regC, global_mean))

    def set_ratings(self, u, j, ctx, r, ctx_ptr=None, ctx_conds=None):
        (u, j, ctx, r), ctx_ptr, ctx_conds = _tuples(u, j, ctx, r), _c32(ctx_ptr), _c32(ctx_conds)
        n_ctx = 0 if ctx_ptr is None else len(ctx_ptr) - 1
        self._chk(self.L.cmi_group_set_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r), n_ctx, _p(ctx_ptr), _p(ctx_conds)))

    def set_state(self, name, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        self._chk(self.L.cmi_group_set_state(self.h, STATE_IDS[name], _p(a), a.size, 1 if a.dtype == np.float64 else 0))

    def set_states(self, state):
        for name, arr in state.items():
            if arr is not None:
                self.set_state(name, arr)

    def get_state(self, name, dtype=np.float64):
        out = np.empty(Instance.state_shape(self, name), dtype=dtype)
        self._chk(self.L.cmi_group_get_state(self.h, STATE_IDS[name], _p(out), out.size, 1 if dtype == np.float64 else 0))
        return out

    def get_states(self, dtype=np.float64):
        return {name: self.get_state(name, dtype) for name in MODEL_STATES[self.model]}

    def set_lr_scale(self, scale):
        self._chk(self.L.cmi_group_set_lr_scale(self.h, float(scale)))

    def train_epoch(self, lrate):
        loss = _dbl()
        self._chk(self.L.cmi_group_train_epoch(self.h, lrate, C.byref(loss)))
        return loss.value

    def train(self, num_iters, init_lrate, max_lrate=-1.0, bold_driver=False, decay=-1.0, early_stop=0, first_iter=1, prev_loss=0.0):
        losses, lrs = np.zeros(num_iters), np.zeros(num_iters)
        n, final = C.c_int(0), _dbl(0)
        rc = self.L.cmi_group_train_from(self.h, first_iter, prev_loss, num_iters, init_lrate, max_lrate, int(bold_driver), decay,
                                         early_stop, _p(losses), _p(lrs), C.byref(n), C.byref(final))
        self.iters_run, self.final_lrate = n.value, final.value
        self._chk(rc)
        return losses[:n.value], lrs[:n.value]

    def eval_ratings(self, u, j, ctx, r, min_rate, max_rate):
        u, j, ctx, r = _tuples(u, j, ctx, r)
        out, cnt = np.zeros(5), _i64()
        self._chk(self.L.cmi_group_eval_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r), min_rate, max_rate, _p(out), C.byref(cnt)))
        return _measures(out, cnt)

    def set_eval_ratings(self, u, j, ctx, r):
        """Test tuples routed once to the shards that own their users and kept on the devices (`--early-stop MAE|RMSE`)."""
        u, j, ctx, r = _tuples(u, j, ctx, r)
        self._chk(self.L.cmi_group_set_eval_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r)))

    def eval_resident(self, min_rate, max_rate):
        out, cnt = np.zeros(5), _i64()
        self._chk(self.L.cmi_group_eval_resident(self.h, min_rate, max_rate, _p(out), C.byref(cnt)))
        return _measures(out, cnt)

    def predict_batch(self, u, j, ctx, bound=False, lo=0.0, hi=0.0):
        u, j, ctx = _tuples(u, j, ctx)
        out = np.empty(len(u))
        self._chk(self.L.cmi_group_predict_batch(self.h, len(u), _p(u), _p(j), _p(ctx), int(bound), lo, hi, _p(out)))
        return out

    def shard_info(self, shard):
        info = (_i64 * 6)()
        self._chk(self.L.cmi_group_shard_info(self.h, shard, info))
        return {"user_lo": info[0], "user_hi": info[1], "tuples": info[2], "device": info[3],
                "exchange": ("none", "rccl", "in-process")[info[4]], "bucket_elems": info[5]}

    def exchange_path(self):
        """Which exchange the group runs and why (RCCL after its pre-flight, or the in-process exchange: shared device / fallback)."""
        return self.L.cmi_group_exchange_path(self.h).decode()

    def last_times(self):
        """(compute_ms, exchange_ms) per shard of the most recent epoch (HIP events on the shards' streams)."""
        W = self.size()
        c, x = (C.c_float * W)(), (C.c_float * W)()
        self._chk(self.L.cmi_group_last_times(self.h, c, x))
        return list(c), list(x)

    def member(self, shard):
        """The shard's instance as a borrowed capi.Instance (the group owns it: do not close)."""
        h = _vp()
        self._chk(self.L.cmi_group_member(self.h, shard, C.byref(h)))
        inst = Instance.__new__(Instance)
        inst.L, inst.h, inst.model, inst.k = self.L, h, self.model, self.k
        si = self.shard_info(shard)
        inst.n_users, inst.n_items, inst.n_conds, inst.num_f, inst.flags = si["user_hi"] - si["user_lo"], self.n_items, self.n_conds, 0, 0
        inst.close = lambda: None
        return inst


class Instance(_Handle):
    """One recommender instance on one GPU (a `cmi_handle`)."""

    _api = ("cmi_create", "cmi_destroy", "cmi_last_error")

    def __init__(self, model, k, n_users, n_items, n_conds, device=0, flags=0):
        self.model = model if isinstance(model, str) else {v: n for n, v in MODEL_IDS.items()}[model]
        self.k, self.n_users, self.n_items, self.n_conds = k, n_users, n_items, n_conds
        self.flags = flags
        self.num_f = 0
        super().__init__(MODEL_IDS[self.model], k, n_users, n_items, n_conds, device, flags)

    # -- data ---------------------------------------------------------------------------------------
    def set_sim_params(self, num_f, n_ctx_dims, empty_conds):
        """CAMF_ICS / LCS / MCS: EmptyContextConditions, `-f` of CAMF_LCS, rateDao.numContextDims() (cmi_set_sim_params)"""
        e = np.ascontiguousarray(empty_conds, dtype=np.int32)
        self._chk(self.L.cmi_set_sim_params(self.h, int(num_f), int(n_ctx_dims), _p(e), len(e)))
        self.num_f = int(num_f)

    def set_ratings(self, u, j, ctx, r, ctx_ptr=None, ctx_conds=None):
        (u, j, ctx, r), ctx_ptr, ctx_conds = _tuples(u, j, ctx, r), _c32(ctx_ptr), _c32(ctx_conds)
        n_ctx = 0 if ctx_ptr is None else len(ctx_ptr) - 1
        self._chk(self.L.cmi_set_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r), n_ctx, _p(ctx_ptr),
                                         _p(ctx_conds)))

    def set_state(self, name, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        self._chk(self.L.cmi_set_state(self.h, STATE_IDS[name], _p(a), a.size, 1 if a.dtype == np.float64 else 0))

    def set_states(self, state):
        for name, arr in state.items():
            if arr is not None:
                self.set_state(name, arr)

    def state_shape(self, name):
        return {"P": (self.n_users, self.k), "Q": (self.n_items, self.k), "userBias": (self.n_users,),
                "itemBias": (self.n_items,), "condBias": (self.n_conds,), "ucBias": (self.n_users, self.n_conds),
                "icBias": (self.n_items, self.n_conds), "Y": (self.n_items, self.k), "ccMatrix": (self.n_conds, self.n_conds),
                "cfMatrix": (self.n_conds, self.num_f), "cVector": (self.n_conds,)}[name]

    def get_state(self, name, dtype=np.float64):
        out = np.empty(self.state_shape(name), dtype=dtype)
        self._chk(self.L.cmi_get_state(self.h, STATE_IDS[name], _p(out), out.size, 1 if dtype == np.float64 else 0))
        return out

    def get_states(self, dtype=np.float64):
        return {name: self.get_state(name, dtype) for name in MODEL_STATES[self.model]}

    def set_hparams(self, regU, regI, regB, regC, global_mean):
        self._chk(self.L.cmi_set_hparams(self.h, regU, regI, regB, regC, global_mean))

    def set_device_share(self, instances):
        """`cv -p on`: how many instances train concurrently on this device (before set_ratings)."""
        self._chk(self.L.cmi_set_device_share(self.h, int(instances)))

    # -- training -----------------------------------------------------------------------------------
    def train_epoch(self, lrate):
        loss = _dbl()
        self._chk(self.L.cmi_train_epoch(self.h, lrate, C.byref(loss)))
        return loss.value

    def train_epoch_async(self, lrate):
        self._chk(self.L.cmi_train_epoch_async(self.h, lrate))

    def last_loss(self):
        loss = _dbl()
        self._chk(self.L.cmi_last_loss(self.h, C.byref(loss)))
        return loss.value

    def train(self, num_iters, init_lrate, max_lrate=-1.0, bold_driver=False, decay=-1.0, early_stop=0, first_iter=1,
              prev_loss=0.0):
        """cmi_train (first_iter == 1) / cmi_train_from: returns (losses, lrates) of the epochs run"""
        losses, lrs = np.zeros(num_iters), np.zeros(num_iters)
        n, final = C.c_int(0), _dbl(0)
        rc = self.L.cmi_train_from(self.h, first_iter, prev_loss, num_iters, init_lrate, max_lrate, int(bold_driver), decay,
                                   early_stop, _p(losses), _p(lrs), C.byref(n), C.byref(final))
        self.iters_run, self.final_lrate = n.value, final.value
        self._chk(rc)
        return losses[:n.value], lrs[:n.value]

    def synchronize(self):
        self._chk(self.L.cmi_synchronize(self.h))

    def stream_ptr(self):
        p = _vp()
        self._chk(self.L.cmi_stream(self.h, C.byref(p)))
        return p.value

    def last_epoch_ms(self):
        ms = C.c_float()
        self._chk(self.L.cmi_last_epoch_ms(self.h, C.byref(ms)))
        return ms.value

    def schedule_info(self):
        info = (_i64 * 8)()
        self._chk(self.L.cmi_schedule_info(self.h, info))
        d = dict(zip(("levels", "max_level", "tuples", "dmax", "state_bytes", "tuple_bytes", "kind", "flow_blocks"),
                     list(info)))
        d["kind"] = ("level", "serial", "flow", "two-lane", "chain-item", "chain-user", "owner-item", "owner-user")[d["kind"]]
        if d["kind"].startswith("owner"):      # owners in the low word, of which teams (three wavefronts each) in the high word
            d["teams"] = d["flow_blocks"] >> 32
            d["flow_blocks"] &= 0xffffffff
        return d

    def schedule_note(self):
        return self.L.cmi_schedule_note(self.h).decode()

    def schedule_traffic(self):
        """HBM bytes per epoch derived from the loaded schedule: {"sector", "own", "algorithmic", "models_reuse"} (cmi_schedule_traffic)"""
        out = (_i64 * 4)()
        self._chk(self.L.cmi_schedule_traffic(self.h, out))
        return {"sector": out[0], "own": out[1], "algorithmic": out[2], "models_reuse": bool(out[3] & 1), "spoke_arena": bool(out[3] & 2)}

    def stream(self):
        s = _vp()
        self._chk(self.L.cmi_stream(self.h, C.byref(s)))
        return s.value

    def save_model(self, path, lrate=0.0, last_loss=0.0, epochs_done=0):
        self._chk(self.L.cmi_save_model(self.h, str(path).encode(), lrate, last_loss, epochs_done))

    def load_model(self, path):
        """-> (lrate, last_loss, epochs_done) stored with the model"""
        lr, ll, ep = C.c_double(), C.c_double(), C.c_int()
        self._chk(self.L.cmi_load_model(self.h, str(path).encode(), C.byref(lr), C.byref(ll), C.byref(ep)))
        if self.model == "CAMF_LCS" and self.n_conds > 0:      # a file may have restored numF into a handle that had none
            self.num_f = self.state_device_ptr("cfMatrix")[1] // self.n_conds
        return lr.value, ll.value, ep.value

    def exchange_setup(self, pad_to=1):
        """(device pointer, element count, numpy dtype) of the item-side exchange bucket; snapshots the current state."""
        ptr, cnt = _vp(), _i64()
        self._chk(self.L.cmi_exchange_setup(self.h, pad_to, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value, (np.float64 if self.flags & FLAG_STATE_F64 else np.float32)

    def exchange_pack(self):
        self._chk(self.L.cmi_exchange_pack(self.h))

    def exchange_apply(self, scale):
        self._chk(self.L.cmi_exchange_apply(self.h, float(scale)))

    def loss_device_ptr(self):
        p = _vp()
        self._chk(self.L.cmi_loss_device_ptr(self.h, C.byref(p)))
        return p.value

    # -- the library's own exchange for one-process-per-GPU jobs (cmi_comm_*: the function cmi_group_* uses) ------------------
    def comm_init(self, unique_id, rank, world):
        """unique_id: COMM_ID_BYTES bytes from comm_unique_id() on rank 0, handed to every rank by the host's rendezvous."""
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.cmi_comm_init(self.h, buf, int(rank), int(world)))

    def comm_last_exchange_ms(self):
        ms = C.c_float()
        self._chk(self.L.cmi_comm_last_exchange_ms(self.h, C.byref(ms)))
        return ms.value

    def comm_exchange(self, scale):
        self._chk(self.L.cmi_comm_exchange(self.h, float(scale)))

    def comm_train_epoch(self, lrate, scale):
        loss = _dbl()
        self._chk(self.L.cmi_comm_train_epoch(self.h, float(lrate), float(scale), C.byref(loss)))
        return loss.value

    def state_device_ptr(self, name):
        ptr, cnt, dt = _vp(), _i64(), C.c_int()
        self._chk(self.L.cmi_state_device_ptr(self.h, STATE_IDS[name], C.byref(ptr), C.byref(cnt), C.byref(dt)))
        return ptr.value, cnt.value, (np.float64 if dt.value else np.float32)

    # -- inference ----------------------------------------------------------------------------------
    def predict(self, u, j, ctx=None, bound=None):
        u, j, ctx = _tuples(u, j, ctx)
        out = np.empty(len(u))
        lo, hi = bound if bound else (0.0, 0.0)
        self._chk(self.L.cmi_predict_batch(self.h, len(u), _p(u), _p(j), _p(ctx), 1 if bound else 0, lo, hi, _p(out)))
        return out

    def eval_ratings(self, u, j, ctx, r, min_rate, max_rate):
        u, j, ctx, r = _tuples(u, j, ctx, r)
        out, cnt = np.zeros(5), _i64()
        self._chk(self.L.cmi_eval_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r), min_rate, max_rate, _p(out),
                                          C.byref(cnt)))
        return _measures(out, cnt)

    def set_eval_ratings(self, u, j, ctx, r):
        """Keep the test tuples on the device for per-epoch evaluation (`--early-stop MAE|RMSE`)."""
        u, j, ctx, r = _tuples(u, j, ctx, r)
        self._chk(self.L.cmi_set_eval_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r)))

    def eval_resident(self, min_rate, max_rate):
        out, cnt = np.zeros(5), _i64()
        self._chk(self.L.cmi_eval_resident(self.h, min_rate, max_rate, _p(out), C.byref(cnt)))
        return _measures(out, cnt)

    def last_rank_ms(self):
        ms, fl = C.c_float(), _dbl()
        self._chk(self.L.cmi_last_rank_ms(self.h, C.byref(ms), C.byref(fl)))
        return ms.value, fl.value

    def last_rank_host_ms(self):
        out = np.zeros(5)
        self._chk(self.L.cmi_last_rank_host_ms(self.h, _p(out)))
        return dict(zip(("plan", "setup", "scoring_loop", "tail", "total"), out.tolist()))

    def last_rank_kernel_ms(self):
        out = np.zeros(2)
        self._chk(self.L.cmi_last_rank_kernel_ms(self.h, _p(out)))
        return dict(zip(("contraction", "selection"), out.tolist()))

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        """Recommender.evalRankings (Recommender.java:668-964).  train/test: (u, j, ctx, r) array tuples.
        Returns {measure: value}; with_lists also returns {(u, ctx): [(item, score), ...]}."""
        return _eval_rankings(self.L.cmi_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)


class FMInstance(_Handle):
    """The reference's FM recommender on one GPU (a `cmi_fm_handle`)."""

    _api = ("cmi_fm_create", "cmi_fm_destroy", "cmi_fm_last_error")

    def __init__(self, k, n_users, n_items, n_conds, n_ctx_dims, device=0, flags=0):
        self.k, self.n_users, self.n_items, self.n_conds = k, n_users, n_items, n_conds
        self.p = n_users + n_items + n_conds
        super().__init__(k, n_users, n_items, n_conds, n_ctx_dims, device, flags)

    def set_hparams(self, regLw, regLf, global_size=0):
        self._chk(self.L.cmi_fm_set_hparams(self.h, regLw, regLf, global_size))

    def set_ratings(self, u, j, ctx, r):
        u, j, ctx, r = _tuples(u, j, ctx, r)
        self._chk(self.L.cmi_fm_set_ratings(self.h, len(r), _p(u), _p(j), _p(ctx), _p(r)))

    def set_model(self, w0, w, V):
        w = np.ascontiguousarray(w, dtype=np.float64).reshape(self.p)
        V = np.ascontiguousarray(V, dtype=np.float64).reshape(self.p, self.k)
        self._chk(self.L.cmi_fm_set_model(self.h, float(w0), _p(w), _p(V)))

    def get_model(self):
        w0, w, V = _dbl(), np.empty(self.p), np.empty((self.p, self.k))
        self._chk(self.L.cmi_fm_get_model(self.h, C.byref(w0), _p(w), _p(V)))
        return w0.value, w, V

    def init(self):
        self._chk(self.L.cmi_fm_init(self.h))

    def sweep(self):
        self._chk(self.L.cmi_fm_sweep(self.h))
        self._chk(self.L.cmi_fm_synchronize(self.h))

    def train(self, num_iters):
        self._chk(self.L.cmi_fm_train(self.h, num_iters))

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        """Recommender.evalRankings with FM.predict as the scorer (see Instance.eval_rankings)."""
        return _eval_rankings(self.L.cmi_fm_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def num_phases(self):
        return self.L.cmi_fm_num_phases(self.h)

    def phase_reduce(self, phase):
        self._chk(self.L.cmi_fm_phase_reduce(self.h, phase))

    def phase_buffer(self, phase):
        ptr, cnt = _vp(), _i64()
        self._chk(self.L.cmi_fm_phase_buffer(self.h, phase, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def phase_run(self, phase):
        self._chk(self.L.cmi_fm_phase_run(self.h, phase))

    def phase_apply(self, phase):
        self._chk(self.L.cmi_fm_phase_apply(self.h, phase))

    def synchronize(self):
        self._chk(self.L.cmi_fm_synchronize(self.h))

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.cmi_fm_comm_init(self.h, buf, int(rank), int(world)))

    def comm_sweep(self):
        self._chk(self.L.cmi_fm_comm_sweep(self.h))

    def layout(self):
        out = np.zeros(12, np.int64)
        self._chk(self.L.cmi_fm_layout(self.h, _p(out)))
        keys = ("slices_user_order", "slices_item_order", "records_user_order", "records_item_order", "records_ctx_order",
                "batches_user_order", "batches_item_order", "bytes_per_factor", "bytes_reduce_user", "bytes_reduce_item",
                "slice_entries", "p")
        return dict(zip(keys, out.tolist()))

    def time_reduce(self, phase, reps=10):
        ms = _dbl()
        self._chk(self.L.cmi_fm_time_reduce(self.h, phase, reps, C.byref(ms)))
        return ms.value

    def stream_ptr(self):
        p = _vp()
        self._chk(self.L.cmi_fm_stream(self.h, C.byref(p)))
        return p.value

    def predict(self, u, j, ctx, bound=None):
        u, j, ctx = _tuples(u, j, ctx)
        out = np.empty(len(u))
        lo, hi = bound if bound else (0.0, 0.0)
        self._chk(self.L.cmi_fm_predict_batch(self.h, len(u), _p(u), _p(j), _p(ctx), 1 if bound else 0, lo, hi, _p(out)))
        return out


KNN_USER, KNN_ITEM = 0, 1
SIM_PCC, SIM_COS, SIM_COS_BINARY, SIM_MSD, SIM_CPC, SIM_EXJACCARD = range(6)


def knn_measure(name):
    """the CMI_SIM_* id of a `similarity` value (case-insensitive; unknown names are pcc, as in the reference)"""
    return lib().cmi_knn_measure(name.encode())


class _PairModel(_Handle):
    """What the pair-co-occurrence handles share: `_prefix` names their C functions (cmi_knn_*, cmi_slope_*, cmi_nmf_*, cmi_slim_*,
    cmi_rankals_*)."""

    _prefix = ""

    def _fn(self, name):
        return getattr(self.L, self._prefix + name)

    def set_ratings(self, u, i, r):
        """the 2-D train matrix as cells (user, item, value)"""
        u = np.ascontiguousarray(u, dtype=np.int32)
        i = np.ascontiguousarray(i, dtype=np.int32)
        r = np.ascontiguousarray(r, dtype=np.float64)
        self._chk(self._fn("_set_ratings")(self.h, len(r), _p(u), _p(i), _p(r)))

    def _predict(self, u, j, *mid, global_mean, bound, lo, hi):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self._fn("_predict_batch")(self.h, len(u), _p(u), _p(j), *mid, float(global_mean), 1 if bound else 0, float(lo),
                                             float(hi), _p(out)))
        return out

    def last_build_ms(self):
        ms = C.c_float()
        self._chk(self._fn("_last_build_ms")(self.h, C.byref(ms)))
        return ms.value

    def _eval_rankings(self, lead, train, test, bin_thold, num_recs, num_ignore, strategy, with_lists):
        """<prefix>_eval_rankings(h, *lead, <the arguments of cmi_slim_eval_rankings>) through the shared helper"""
        fn = self._fn("_eval_rankings")
        return _eval_rankings(lambda h, *rest: fn(h, *lead, *rest), self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_rank_ms(self):
        """device milliseconds of the scoring and selection of the last eval_rankings()"""
        ms = C.c_float()
        self._chk(self._fn("_last_rank_ms")(self.h, C.byref(ms)))
        return ms.value


class KNNInstance(_PairModel):
    """The reference's ItemKNN (kind="item") or UserKNN (kind="user") on one GPU (a `cmi_knn_handle`)."""

    _api = ("cmi_knn_create", "cmi_knn_destroy", "cmi_knn_last_error")
    _prefix = "cmi_knn"

    def __init__(self, kind, n_users, n_items, device=0, flags=0):
        k = {"user": KNN_USER, "item": KNN_ITEM}.get(kind, kind)
        self.kind, self.n_users, self.n_items = k, n_users, n_items
        self.n = n_items if k == KNN_ITEM else n_users
        super().__init__(k if isinstance(k, int) else -1, n_users, n_items, device, flags)

    def build(self, measure="pcc", shrinkage=-1, min_rate=1.0, max_rate=5.0):
        m = knn_measure(measure) if isinstance(measure, str) else int(measure)
        self._chk(self.L.cmi_knn_build(self.h, m, int(shrinkage), float(min_rate), float(max_rate)))

    def similarity(self, row0=0, nrows=None):
        """rows of the dense similarity matrix (NaN where unset)"""
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty((max(nrows, 0), self.n))
        self._chk(self.L.cmi_knn_get_similarity(self.h, int(row0), int(nrows), _p(out)))
        return out

    def predict(self, u, j, knn, global_mean, bound=False, lo=1.0, hi=5.0):
        return self._predict(u, j, int(knn), global_mean=global_mean, bound=bound, lo=lo, hi=hi)

    def ranking(self, u, j, knn, global_mean):
        """Recommender.ranking(u, j): predict under isRankingPred (a neighbour needs a set, non-zero similarity of either sign), unbounded"""
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_knn_ranking_batch(self.h, len(u), _p(u), _p(j), int(knn), float(global_mean), _p(out)))
        return out

    def eval_rankings(self, train, test, knn, global_mean, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        """Recommender.evalRankings with ranking() as the scorer; keywords and return as SLIMInstance.eval_rankings"""
        return self._eval_rankings((int(knn), float(global_mean)), train, test, bin_thold, num_recs, num_ignore, strategy, with_lists)


class SlopeOneInstance(_PairModel):
    """The reference's SlopeOne on one GPU (a `cmi_slope_handle`)."""

    _api = ("cmi_slope_create", "cmi_slope_destroy", "cmi_slope_last_error")
    _prefix = "cmi_slope"

    def __init__(self, n_users, n_items, device=0, flags=0):
        self.n_users, self.n_items = n_users, n_items
        super().__init__(n_users, n_items, device, flags)

    def build(self):
        self._chk(self.L.cmi_slope_build(self.h))

    def deviation(self, row0=0, nrows=None):
        """rows of the dense deviation (fp64) and cardinality (int32) matrices: (dev, card)"""
        nrows = self.n_items - row0 if nrows is None else nrows
        dev = np.empty((max(nrows, 0), self.n_items))
        card = np.empty((max(nrows, 0), self.n_items), np.int32)
        self._chk(self.L.cmi_slope_get_deviation(self.h, int(row0), int(nrows), _p(dev), _p(card)))
        return dev, card

    def predict(self, u, j, global_mean, bound=False, lo=1.0, hi=5.0):
        return self._predict(u, j, global_mean=global_mean, bound=bound, lo=lo, hi=hi)

    def eval_rankings(self, train, test, global_mean, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        """Recommender.evalRankings with the unbounded predict as the scorer; keywords and return as SLIMInstance.eval_rankings"""
        return self._eval_rankings((float(global_mean),), train, test, bin_thold, num_recs, num_ignore, strategy, with_lists)


class _FactorModel(_PairModel):
    """What the handles of a k-factor model of the 2-D train matrix share (cmi_nmf_*, cmi_rankals_*): create(k, n_users, n_items, ...)
    and the shape check of an injected factor matrix."""

    def __init__(self, k, n_users, n_items, device=0, flags=0):
        self.k, self.n_users, self.n_items = k, n_users, n_items
        super().__init__(k, n_users, n_items, device, flags)

    def _shaped(self, a, shape, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != shape:
            raise CmiError(E_INVALID, "%s has shape %s, not %s" % (name, a.shape, shape))
        return a


class NMFInstance(_FactorModel):
    """The reference's NMF on one GPU (a `cmi_nmf_handle`): W is (n_users, k), H is (k, n_items), 1 <= k <= 256."""

    _api = ("cmi_nmf_create", "cmi_nmf_destroy", "cmi_nmf_last_error")
    _prefix = "cmi_nmf"

    def set_model(self, W=None, H=None):
        W = self._shaped(W, (self.n_users, self.k), "W")
        H = self._shaped(H, (self.k, self.n_items), "H")
        self._chk(self.L.cmi_nmf_set_model(self.h, None if W is None else _p(W), None if H is None else _p(H)))

    def model(self):
        """(W, H)"""
        W, H = np.empty((self.n_users, self.k)), np.empty((self.k, self.n_items))
        self._chk(self.L.cmi_nmf_get_model(self.h, _p(W), _p(H)))
        return W, H

    def iterate(self):
        """one W phase, H phase and loss; returns the loss (a NaN / Inf loss raises E_NUMERIC)"""
        loss = _dbl()
        self._chk(self.L.cmi_nmf_iterate(self.h, C.byref(loss)))
        return loss.value

    def predict(self, u, j, bound=False, lo=1.0, hi=5.0):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_nmf_predict_batch(self.h, len(u), _p(u), _p(j), 1 if bound else 0, float(lo), float(hi), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        """Recommender.evalRankings with the unbounded predict as the scorer (k <= 128); keywords and return as SLIMInstance.eval_rankings"""
        return _eval_rankings(self.L.cmi_topn_nmf_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_rank_ms(self):
        """device milliseconds of the scoring and selection of the last eval_rankings()"""
        ms = C.c_float()
        self._chk(self.L.cmi_topn_nmf_last_rank_ms(self.h, C.byref(ms)))
        return ms.value

    def last_iter_ms(self):
        """(W phase, H phase, loss) device milliseconds of the last iterate()"""
        ms = (C.c_float * 3)()
        self._chk(self.L.cmi_nmf_last_iter_ms(self.h, ms))
        return tuple(ms)


def slim_cut_neighbors(sims, knn):
    """Host-only: the neighbour list SLIM.initModel makes of one item's similarity row (NaN unset), in its iteration order
    (see cmi_slim_cut_neighbors); E_UNSUPPORTED when a hash bin would treeify"""
    sims = np.ascontiguousarray(sims, dtype=np.float64)
    out, n = np.empty(max(len(sims), 1), np.int32), C.c_int32()
    rc = lib().cmi_slim_cut_neighbors(len(sims), _p(sims), int(knn), _p(out), C.byref(n))
    if rc != OK:
        raise CmiError(rc, (lib().cmi_last_error(None) or b"cmi_slim_cut_neighbors").decode())
    return out[:n.value].tolist()


class SLIMInstance(_PairModel):
    """The reference's SLIM on one GPU (a `cmi_slim_handle`): per item a neighbour list in the reference's iteration order and one
    weight per list entry, W[i][j]."""

    _api = ("cmi_slim_create", "cmi_slim_destroy", "cmi_slim_last_error")
    _prefix = "cmi_slim"

    def __init__(self, n_users, n_items, device=0, flags=0):
        self.n_users, self.n_items = n_users, n_items
        super().__init__(n_users, n_items, device, flags)

    def build_neighbors(self, knn, measure="pcc", shrinkage=-1, min_rate=1.0, max_rate=5.0):
        m = knn_measure(measure) if isinstance(measure, str) else int(measure)
        self._chk(self.L.cmi_slim_build_neighbors(self.h, int(knn), m, int(shrinkage), float(min_rate), float(max_rate)))

    def neighbors(self):
        """(ptr, idx): item j's list is idx[ptr[j]:ptr[j + 1]]"""
        ptr = np.empty(self.n_items + 1, np.int64)
        self._chk(self.L.cmi_slim_get_neighbors(self.h, _p(ptr), None))
        idx = np.empty(int(ptr[-1]), np.int32)
        self._chk(self.L.cmi_slim_get_neighbors(self.h, _p(ptr), _p(idx)))
        return ptr, idx

    def set_weights(self, w):
        """w[p] = W[idx[p]][j], aligned with neighbors()'s idx"""
        ptr = np.empty(self.n_items + 1, np.int64)
        self._chk(self.L.cmi_slim_get_neighbors(self.h, _p(ptr), None))
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.shape != (int(ptr[-1]),):
            raise CmiError(E_INVALID, "w has shape %s, not (%d,)" % (w.shape, int(ptr[-1])))
        self._chk(self.L.cmi_slim_set_weights(self.h, _p(w)))

    def weights(self):
        ptr = np.empty(self.n_items + 1, np.int64)
        self._chk(self.L.cmi_slim_get_neighbors(self.h, _p(ptr), None))
        w = np.empty(int(ptr[-1]))
        self._chk(self.L.cmi_slim_get_weights(self.h, _p(w)))
        return w

    def iterate(self, l1, l2):
        """one pass over every coordinate; l1, l2: the doubles of the reference's floats.  Returns the loss (NaN / Inf raises E_NUMERIC)"""
        loss = _dbl()
        self._chk(self.L.cmi_slim_iterate(self.h, float(l1), float(l2), C.byref(loss)))
        return loss.value

    def predict(self, u, j):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_slim_predict_batch(self.h, len(u), _p(u), _p(j), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_slim_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_iter_ms(self):
        """(sweep, loss chain) device milliseconds of the last iterate()"""
        ms = (C.c_float * 2)()
        self._chk(self.L.cmi_slim_last_iter_ms(self.h, ms))
        return tuple(ms)


class RankALSInstance(_FactorModel):
    """The reference's RankALS on one GPU (a `cmi_rankals_handle`): P is (n_users, k), Q is (n_items, k), 1 <= k <= 64."""

    _api = ("cmi_rankals_create", "cmi_rankals_destroy", "cmi_rankals_last_error")
    _prefix = "cmi_rankals"

    def set_model(self, P=None, Q=None):
        P = self._shaped(P, (self.n_users, self.k), "P")
        Q = self._shaped(Q, (self.n_items, self.k), "Q")
        self._chk(self.L.cmi_rankals_set_model(self.h, None if P is None else _p(P), None if Q is None else _p(Q)))

    def model(self):
        """(P, Q)"""
        P, Q = np.empty((self.n_users, self.k)), np.empty((self.n_items, self.k))
        self._chk(self.L.cmi_rankals_get_model(self.h, _p(P), _p(Q)))
        return P, Q

    def iterate(self, support_weight):
        """one pass of buildModel's loop: the P step over the users of rows(), the Q step over every item"""
        self._chk(self.L.cmi_rankals_iterate(self.h, 1 if support_weight else 0))

    def predict(self, u, j):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_rankals_predict_batch(self.h, len(u), _p(u), _p(j), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_rankals_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_iter_ms(self):
        """(item moments, user solves, user moments, item solves) device milliseconds of the last iterate() and the scoring loop of the
        last eval_rankings(); 0.0 for whichever of the two has not run yet"""
        ms = (C.c_float * 5)()
        self._chk(self.L.cmi_rankals_last_iter_ms(self.h, ms))
        return tuple(ms)

    def invert(self, A):
        """librec's DenseMatrix.inv() of a batch of square matrices, shape (n_mats, n, n), by the device routine the solves use"""
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise CmiError(E_INVALID, "A has shape %s, not (n_mats, n, n)" % (A.shape,))
        out = np.empty_like(A)
        self._chk(self.L.cmi_rankals_invert(self.h, A.shape[0], A.shape[1], _p(A), _p(out)))
        return out


BPR_FLAG_STRICT, BPR_FLAG_HOST_SAMPLER, BPR_FLAG_MIN_SLACK = 0x1, 0x2, 0x4
JAVA_LCG_MASK = (1 << 48) - 1


def java_random_state(seed):
    """the 48-bit state of `new java.util.Random(seed)`"""
    return (int(seed) ^ 0x5DEECE66D) & JAVA_LCG_MASK


def _bpr_chk(rc, fn):
    if rc != OK:
        raise CmiError(rc, (lib().cmi_bpr_last_error(None) or fn.encode()).decode())


def java_next_ints(state, bound, n, on_device=False):
    """Host-only unless on_device: n values of java.util.Random.nextInt(bound) from the 48-bit `state`; (values, state after)"""
    st, out = _i64(int(state)), np.empty(max(int(n), 1), np.int32)
    _bpr_chk(lib().cmi_java_next_ints(C.byref(st), int(bound), int(n), _p(out), 1 if on_device else 0), "cmi_java_next_ints")
    return out[:int(n)], st.value


def java_exp_log(x, on_device=False):
    """Host-only unless on_device: (StrictMath.exp(x), StrictMath.log(x)), fdlibm's algorithms"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    e, l = np.empty(max(len(x), 1)), np.empty(max(len(x), 1))
    _bpr_chk(lib().cmi_java_exp_log(len(x), _p(x), _p(e), _p(l), 1 if on_device else 0), "cmi_java_exp_log")
    return e[:len(x)], l[:len(x)]


def bpr_levels(n_users, n_items, u, i, j):
    """Host-only: BPR's level schedule of the triples: (order, level_of, n_levels, max_chain)"""
    u = np.ascontiguousarray(u, dtype=np.int32)
    i = np.ascontiguousarray(i, dtype=np.int32)
    j = np.ascontiguousarray(j, dtype=np.int32)
    order, level_of = np.empty(max(len(u), 1), np.int32), np.empty(max(len(u), 1), np.int32)
    nl, chain = _i32(), _i64()
    _bpr_chk(lib().cmi_bpr_levels(int(n_users), int(n_items), len(u), _p(u), _p(i), _p(j), _p(order), _p(level_of), C.byref(nl),
                                  C.byref(chain)), "cmi_bpr_levels")
    return order[:len(u)], level_of[:len(u)], nl.value, chain.value


def bpr_sample_host(n_users, n_items, u, i, r, state, n_samples):
    """Host-only: BPR.java's sequential sampler over the cells' matrix from the 48-bit `state`: (u, i, j, state after)"""
    u = np.ascontiguousarray(u, dtype=np.int32)
    i = np.ascontiguousarray(i, dtype=np.int32)
    r = np.ascontiguousarray(r, dtype=np.float64)
    st = _i64(int(state))
    ou, oi, oj = (np.empty(max(int(n_samples), 1), np.int32) for _ in range(3))
    _bpr_chk(lib().cmi_bpr_sample_host(int(n_users), int(n_items), len(r), _p(u), _p(i), _p(r), C.byref(st), int(n_samples), _p(ou),
                                       _p(oi), _p(oj)), "cmi_bpr_sample_host")
    n = int(n_samples)
    return ou[:n], oi[:n], oj[:n], st.value


class BPRInstance(_FactorModel):
    """The reference's BPR on one GPU (a `cmi_bpr_handle`): P is (n_users, k), Q is (n_items, k), 1 <= k <= 128."""

    _api = ("cmi_bpr_create", "cmi_bpr_destroy", "cmi_bpr_last_error")
    _prefix = "cmi_bpr"

    def set_model(self, P=None, Q=None):
        P = self._shaped(P, (self.n_users, self.k), "P")
        Q = self._shaped(Q, (self.n_items, self.k), "Q")
        self._chk(self.L.cmi_bpr_set_model(self.h, None if P is None else _p(P), None if Q is None else _p(Q)))

    def model(self):
        """(P, Q)"""
        P, Q = np.empty((self.n_users, self.k)), np.empty((self.n_items, self.k))
        self._chk(self.L.cmi_bpr_get_model(self.h, _p(P), _p(Q)))
        return P, Q

    def set_random_state(self, state):
        self._chk(self.L.cmi_bpr_set_random_state(self.h, int(state)))

    def random_state(self):
        st = _i64()
        self._chk(self.L.cmi_bpr_get_random_state(self.h, C.byref(st)))
        return st.value

    def sample(self, on_device=True):
        """one iteration's triples from the current stream state, which stays: (u, i, j, state after)"""
        n = self.n_users * 100
        u, i, j, st = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), _i64()
        self._chk(self.L.cmi_bpr_sample(self.h, 1 if on_device else 0, _p(u), _p(i), _p(j), C.byref(st)))
        return u, i, j, st.value

    def iterate(self, lrate, reg_u, reg_i):
        """one iteration of buildModel's loop (sample, level build, epoch, loss); returns the loss (NaN / Inf raises E_NUMERIC)"""
        loss = _dbl()
        self._chk(self.L.cmi_bpr_iterate(self.h, float(lrate), float(reg_u), float(reg_i), C.byref(loss)))
        return loss.value

    def predict(self, u, j):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_bpr_predict_batch(self.h, len(u), _p(u), _p(j), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_bpr_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_iter_ms(self):
        """(sampler, level build, epoch, loss) milliseconds of the last iterate() -- the first two host wall time, the others device
        time -- and the scoring loop of the last eval_rankings(); 0.0 for whichever of the two has not run yet"""
        ms = (C.c_float * 5)()
        self._chk(self.L.cmi_bpr_last_iter_ms(self.h, ms))
        return tuple(ms)

    def last_schedule(self):
        out = (_i64 * 5)()
        self._chk(self.L.cmi_bpr_last_schedule(self.h, out))
        return dict(zip(("levels", "alone", "runs", "widest", "sampler_fallbacks"), (int(x) for x in out)))


RANKSGD_FLAG_STRICT, RANKSGD_FLAG_HOST_SAMPLER, RANKSGD_FLAG_NUM_RATES_SIZE = 0x1, 0x2, 0x4


def _ranksgd_chk(rc, fn):
    if rc != OK:
        raise CmiError(rc, (lib().cmi_ranksgd_last_error(None) or fn.encode()).decode())


def _ranksgd_cells(u, i, r):
    return (np.ascontiguousarray(u, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32), np.ascontiguousarray(r, dtype=np.float64))


def ranksgd_item_table(n_users, n_items, u, i, r, flags=0):
    """Host-only: RankSGD.java:66-75 of the cells' matrix: (the list's items, the running sums along it).  flags: 0 divides by the
    reference's unassigned numRates (0), RANKSGD_FLAG_NUM_RATES_SIZE by the number of non-zero cells"""
    u, i, r = _ranksgd_cells(u, i, r)
    item, cum, n = np.empty(max(int(n_items), 1), np.int32), np.empty(max(int(n_items), 1)), _i32()
    _ranksgd_chk(lib().cmi_ranksgd_item_table(int(n_users), int(n_items), len(r), _p(u), _p(i), _p(r), int(flags), _p(item), _p(cum),
                                              C.byref(n)), "cmi_ranksgd_item_table")
    return item[:n.value], cum[:n.value]


def ranksgd_tries(state, item, cum, n, on_device=False):
    """Host-only unless on_device: the item (or -1) of the n tries that start 0, 2, 4, ... draws after the 48-bit `state`"""
    item, cum = np.ascontiguousarray(item, dtype=np.int32), np.ascontiguousarray(cum, dtype=np.float64)
    out = np.empty(max(int(n), 1), np.int32)
    _ranksgd_chk(lib().cmi_ranksgd_tries(int(state), len(item), _p(item), _p(cum), int(n), _p(out), 1 if on_device else 0),
                 "cmi_ranksgd_tries")
    return out[:int(n)]


def ranksgd_assign_host(n_users, n_items, u, i, r, try_item):
    """Host-only: RankSGD.java:85-112 with the tries given: (j per non-zero cell in cell order, tries consumed)"""
    u, i, r = _ranksgd_cells(u, i, r)
    tries = np.ascontiguousarray(try_item, dtype=np.int32)
    j, used = np.empty(max(len(r), 1), np.int32), _i64()
    _ranksgd_chk(lib().cmi_ranksgd_assign_host(int(n_users), int(n_items), len(r), _p(u), _p(i), _p(r), len(tries), _p(tries), _p(j),
                                               C.byref(used)), "cmi_ranksgd_assign_host")
    return j[:int(np.count_nonzero(r))], used.value


def ranksgd_sample_host(n_users, n_items, u, i, r, state, flags=0):
    """Host-only: one iteration's samples of the cells' matrix from the 48-bit `state`: (u, i, j, rui, state after, tries consumed)"""
    u, i, r = _ranksgd_cells(u, i, r)
    n = max(len(r), 1)
    ou, oi, oj, orr = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
    st, cells, used = _i64(int(state)), _i64(), _i64()
    _ranksgd_chk(lib().cmi_ranksgd_sample_host(int(n_users), int(n_items), len(r), _p(u), _p(i), _p(r), int(flags), C.byref(st), _p(ou),
                                               _p(oi), _p(oj), _p(orr), C.byref(cells), C.byref(used)), "cmi_ranksgd_sample_host")
    c = cells.value
    return ou[:c], oi[:c], oj[:c], orr[:c], st.value, used.value


class RankSGDInstance(_FactorModel):
    """The reference's RankSGD on one GPU (a `cmi_ranksgd_handle`): P is (n_users, k), Q is (n_items, k), 1 <= k <= 128."""

    _api = ("cmi_ranksgd_create", "cmi_ranksgd_destroy", "cmi_ranksgd_last_error")
    _prefix = "cmi_ranksgd"

    def set_ratings(self, u, i, r):
        super().set_ratings(u, i, r)
        self.n_cells = int(np.count_nonzero(np.asarray(r, dtype=np.float64)))

    def set_model(self, P=None, Q=None):
        P = self._shaped(P, (self.n_users, self.k), "P")
        Q = self._shaped(Q, (self.n_items, self.k), "Q")
        self._chk(self.L.cmi_ranksgd_set_model(self.h, None if P is None else _p(P), None if Q is None else _p(Q)))

    def model(self):
        """(P, Q)"""
        P, Q = np.empty((self.n_users, self.k)), np.empty((self.n_items, self.k))
        self._chk(self.L.cmi_ranksgd_get_model(self.h, _p(P), _p(Q)))
        return P, Q

    def set_random_state(self, state):
        self._chk(self.L.cmi_ranksgd_set_random_state(self.h, int(state)))

    def random_state(self):
        st = _i64()
        self._chk(self.L.cmi_ranksgd_get_random_state(self.h, C.byref(st)))
        return st.value

    def sample(self, on_device=True, max_device_tries=0):
        """one iteration's samples from the current stream state, which stays: (u, i, j, rui, state after)"""
        n = max(getattr(self, "n_cells", 0), 1)
        u, i, j, r, st = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n), _i64()
        self._chk(self.L.cmi_ranksgd_sample(self.h, 1 if on_device else 0, int(max_device_tries), _p(u), _p(i), _p(j), _p(r), C.byref(st)))
        c = getattr(self, "n_cells", 0)
        return u[:c], i[:c], j[:c], r[:c], st.value

    def iterate(self, lrate):
        """one iteration of buildModel's loop (tries, walk, level build, epoch, loss); returns the loss"""
        loss = _dbl()
        self._chk(self.L.cmi_ranksgd_iterate(self.h, float(lrate), C.byref(loss)))
        return loss.value

    def predict(self, u, j):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_ranksgd_predict_batch(self.h, len(u), _p(u), _p(j), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_ranksgd_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_iter_ms(self):
        """(device tries, host walk, level build, epoch, loss) milliseconds of the last iterate() -- the first three host wall time, the
        others device time -- and the scoring loop of the last eval_rankings()"""
        ms = (C.c_float * 6)()
        self._chk(self.L.cmi_ranksgd_last_iter_ms(self.h, ms))
        return tuple(ms)

    def last_schedule(self):
        out = (_i64 * 5)()
        self._chk(self.L.cmi_ranksgd_last_schedule(self.h, out))
        return dict(zip(("levels", "alone", "runs", "widest", "host_tries"), (int(x) for x in out)))


LRMF_FLAG_STRICT, LRMF_FLAG_GLOBAL_ROWS = 0x1, 0x2


def lrmf_lds_rows(k):
    """Host-only: the most cells of a unit that keeps its item rows in LDS at k factors"""
    return int(lib().cmi_lrmf_lds_rows(int(k)))


def lrmf_block():
    """Host-only: the threads of an LRMF workgroup, the item lanes of one pass of a cell's sum"""
    return int(lib().cmi_lrmf_block())


def lrmf_levels(n_users, n_items, u, i):
    """Host-only: LRMF's unit schedule of the cells: (order, level_of, n_levels, max_chain); order holds the users that store a cell"""
    u = np.ascontiguousarray(u, dtype=np.int32)
    i = np.ascontiguousarray(i, dtype=np.int32)
    order, level_of = np.empty(max(int(n_users), 1), np.int32), np.zeros(max(int(n_users), 1), np.int32)
    nl, chain = _i32(), _i64()
    rc = lib().cmi_lrmf_levels(int(n_users), int(n_items), len(u), _p(u), _p(i), _p(order), _p(level_of), C.byref(nl), C.byref(chain))
    if rc != OK:
        raise CmiError(rc, (lib().cmi_lrmf_last_error(None) or b"cmi_lrmf_levels").decode())
    level_of = level_of[:max(int(n_users), 0)]
    return order[:int(np.count_nonzero(level_of))], level_of, nl.value, chain.value


class LRMFInstance(_FactorModel):
    """The reference's LRMF on one GPU (a `cmi_lrmf_handle`): P is (n_users, k), Q is (n_items, k), 1 <= k <= 128."""

    _api = ("cmi_lrmf_create", "cmi_lrmf_destroy", "cmi_lrmf_last_error")
    _prefix = "cmi_lrmf"

    def set_model(self, P=None, Q=None):
        P = self._shaped(P, (self.n_users, self.k), "P")
        Q = self._shaped(Q, (self.n_items, self.k), "Q")
        self._chk(self.L.cmi_lrmf_set_model(self.h, None if P is None else _p(P), None if Q is None else _p(Q)))

    def model(self):
        """(P, Q)"""
        P, Q = np.empty((self.n_users, self.k)), np.empty((self.n_items, self.k))
        self._chk(self.L.cmi_lrmf_get_model(self.h, _p(P), _p(Q)))
        return P, Q

    def iterate(self, lrate, reg_u, reg_i):
        """one iteration of buildModel's loop (epoch, loss); returns the loss (NaN / Inf raises E_NUMERIC)"""
        loss = _dbl()
        self._chk(self.L.cmi_lrmf_iterate(self.h, float(lrate), float(reg_u), float(reg_i), C.byref(loss)))
        return loss.value

    def predict(self, u, j):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_lrmf_predict_batch(self.h, len(u), _p(u), _p(j), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_lrmf_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore,
                              strategy, with_lists)

    def last_iter_ms(self):
        """(epoch, loss) device milliseconds of the last iterate() and the scoring loop of the last eval_rankings(); 0.0 for whichever
        of the two has not run yet"""
        ms = (C.c_float * 3)()
        self._chk(self.L.cmi_lrmf_last_iter_ms(self.h, ms))
        return tuple(ms)

    def last_schedule(self):
        out = (_i64 * 5)()
        self._chk(self.L.cmi_lrmf_last_schedule(self.h, out))
        return dict(zip(("levels", "alone", "runs", "widest", "global_units"), (int(x) for x in out)))


CPTF_FLAG_STRICT, CPTF_FLAG_GLOBAL_CTX, CPTF_FLAG_KEYS_INDEXOF = 0x1, 0x2, 0x4


def cptf_tensor_build(cells, pair_user, pair_item, ctx_conds, cond_dim, test_pairs=(), flags=0):
    """Host-only: DataDAO.toSparseTensor, TensorRecommender's fold split and getKeys.  cells: (pair, context, rate) in rateMatrix
    order; ctx_conds[c]: the context's conditions in list order; cond_dim[cond]: its dimension; test_pairs: the pair of every cell
    of testMatrix in its order.  flags: 0 the reference's keys, CPTF_FLAG_KEYS_INDEXOF the condition's own index.
    Returns a dict: dims, dim_lists, keys, vals, train_keys, train_vals, test_keys, test_vals, ctx_keys"""
    pair = np.ascontiguousarray([c[0] for c in cells], dtype=np.int32)
    ctx = np.ascontiguousarray([c[1] for c in cells], dtype=np.int32)
    rate = np.ascontiguousarray([c[2] for c in cells], dtype=np.float64)
    pu, pi = _c32(pair_user), _c32(pair_item)
    ptr = np.zeros(len(ctx_conds) + 1, np.int32)
    ptr[1:] = np.cumsum([len(c) for c in ctx_conds])
    conds = np.ascontiguousarray([x for c in ctx_conds for x in c], dtype=np.int32)
    cd, tp = _c32(cond_dim), _c32(list(test_pairs))
    n, D = len(cells), (int(cd.max()) + 1 if len(cd) else 0)
    nd = C.c_int32()
    dims, lptr, lst = np.zeros(16, np.int32), np.zeros(D + 2, np.int32), np.zeros(max(len(cd), 1), np.int32)
    room = max(n, 1) * max(2 + D, 2)
    keys, trk, tek = (np.zeros(room, np.int32) for _ in range(3))
    vals, trv, tev = (np.zeros(max(n, 1)) for _ in range(3))
    ntr, nte = _i64(), _i64()
    ck = np.zeros(max(len(ctx_conds) * D, 1), np.int32)
    rc = lib().cmi_cptf_tensor_build(n, _p(pair), _p(ctx), _p(rate), len(pu), _p(pu), _p(pi), len(ctx_conds), _p(ptr), _p(conds), len(cd),
                                     _p(cd), len(tp), _p(tp), int(flags), C.byref(nd), _p(dims), _p(lptr), _p(lst), _p(keys), _p(vals),
                                     C.byref(ntr), _p(trk), _p(trv), C.byref(nte), _p(tek), _p(tev), _p(ck))
    if rc != OK:
        raise CmiError(rc, lib().cmi_cptf_last_error(None).decode())
    w = nd.value
    return {"dims": dims[:w].tolist(), "dim_lists": [lst[lptr[d]:lptr[d + 1]].tolist() for d in range(w - 2)],
            "keys": keys[:n * w].reshape(n, w).copy(), "vals": vals[:n].copy(),
            "train_keys": trk[:ntr.value * w].reshape(-1, w).copy(), "train_vals": trv[:ntr.value].copy(),
            "test_keys": tek[:nte.value * w].reshape(-1, w).copy(), "test_vals": tev[:nte.value].copy(),
            "ctx_keys": ck[:len(ctx_conds) * (w - 2)].reshape(len(ctx_conds), w - 2).copy()}


class CPTFInstance(_Handle):
    """The reference's CPTF on one GPU (a `cmi_cptf_handle`): one factor matrix (dims[d], k) per tensor dimension -- user, item, then
    one per context dimension.  1 <= k <= 128, 2 <= len(dims) <= 10."""

    _api = ("cmi_cptf_create", "cmi_cptf_destroy", "cmi_cptf_last_error")

    def __init__(self, k, dims, device=0, flags=0):
        self.k, self.dims = k, [int(d) for d in dims]
        self.n_users, self.n_items = (self.dims + [0, 0])[:2]
        d = np.ascontiguousarray(self.dims, dtype=np.int32)
        super().__init__(k, len(self.dims), _p(d), device, flags)

    def _keys(self, keys, width):
        keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1, width) if width else np.zeros((len(keys), 0), np.int32)
        return np.ascontiguousarray(keys)

    def set_entries(self, keys, r):
        """trainTensor in iterator order: keys (n, len(dims)) and the rates"""
        keys, r = self._keys(keys, len(self.dims)), np.ascontiguousarray(r, dtype=np.float64)
        if len(keys) != len(r):
            raise CmiError(E_INVALID, "%d key tuples for %d rates" % (len(keys), len(r)))
        self._chk(self.L.cmi_cptf_set_entries(self.h, len(r), _p(keys), _p(r)))

    def set_context_keys(self, ctx_keys):
        """TensorRecommender.getKeys' keys of every context id: (n_ctx, len(dims) - 2)"""
        ctx_keys = self._keys(ctx_keys, len(self.dims) - 2)
        self._chk(self.L.cmi_cptf_set_context_keys(self.h, len(ctx_keys), _p(ctx_keys)))

    def set_rating_range(self, min_rate, max_rate):
        self._chk(self.L.cmi_cptf_set_rating_range(self.h, float(min_rate), float(max_rate)))

    def set_model(self, M):
        """M: one (dims[d], k) matrix per dimension"""
        if len(M) != len(self.dims):
            raise CmiError(E_INVALID, "%d matrices for %d dimensions" % (len(M), len(self.dims)))
        parts = []
        for d, a in enumerate(M):
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (self.dims[d], self.k):
                raise CmiError(E_INVALID, "M[%d] has shape %s, not %s" % (d, a.shape, (self.dims[d], self.k)))
            parts.append(a.ravel())
        flat = np.ascontiguousarray(np.concatenate(parts))
        self._chk(self.L.cmi_cptf_set_model(self.h, _p(flat)))

    def model(self):
        """[M[0], ..., M[len(dims) - 1]]"""
        flat = np.empty(sum(self.dims) * self.k)
        self._chk(self.L.cmi_cptf_get_model(self.h, _p(flat)))
        out, at = [], 0
        for n in self.dims:
            out.append(flat[at:at + n * self.k].reshape(n, self.k).copy())
            at += n * self.k
        return out

    def iterate(self, lrate, reg):
        """one iteration of CPTF.buildModel's loop; returns the loss (a CmiError of code E_NUMERIC carries a non-finite one as .loss)"""
        loss = _dbl()
        rc = self.L.cmi_cptf_iterate(self.h, float(lrate), float(reg), C.byref(loss))
        if rc != OK:
            err = CmiError(rc, self.L.cmi_cptf_last_error(self.h).decode())
            err.loss = loss.value
            raise err
        return loss.value

    def predict(self, keys, bound=False, lo=0.0, hi=0.0):
        """CPTF.predict(keys) of (n, len(dims)) key tuples; bound: clamped to [lo, hi]"""
        keys = self._keys(keys, len(self.dims))
        out = np.empty(len(keys))
        self._chk(self.L.cmi_cptf_predict_batch(self.h, len(keys), _p(keys), 1 if bound else 0, float(lo), float(hi), _p(out)))
        return out

    def eval_rankings(self, train, test, bin_thold=-1.0, num_recs=10, num_ignore=0, strategy="ucu", with_lists=False):
        return _eval_rankings(self.L.cmi_cptf_eval_rankings, self._chk, self.h, train, test, bin_thold, num_recs, num_ignore, strategy,
                              with_lists)

    def last_iter_ms(self):
        """(epoch, loss sum) device milliseconds of the last iterate() and the scoring loop of the last eval_rankings()"""
        ms = (C.c_float * 3)()
        self._chk(self.L.cmi_cptf_last_iter_ms(self.h, ms))
        return tuple(ms)

    def ctx_in_lds(self):
        return bool(self.L.cmi_cptf_ctx_in_lds(self.h))


BPMF_FLAG_STRICT = 0x1
BPMF_MAX_K, BPMF_BLOCK, BPMF_TILE, BPMF_CHUNK, BPMF_GAUSS_BLOCK, BPMF_STAGE_MIN = 64, 256, 32, 64, 256, 1024   # bpmf_kernels.hpp


def _bpmf_chk(rc, fn):
    if rc != OK:
        raise CmiError(rc, (lib().cmi_bpmf_last_error(None) or fn.encode()).decode())


def java_next_gaussians(state, n, have_cached=False, cached=0.0):
    """n values of java.util.Random.nextGaussian() on the device from the 48-bit `state` and the cached second value of the last pair;
    (values, (state, have_cached, cached) after)"""
    st, hv, cv = _i64(int(state)), C.c_int(1 if have_cached else 0), _dbl(float(cached))
    out = np.empty(max(int(n), 1))
    _bpmf_chk(lib().cmi_java_next_gaussians(C.byref(st), C.byref(hv), C.byref(cv), int(n), _p(out)), "cmi_java_next_gaussians")
    return out[:int(n)], (st.value, bool(hv.value), cv.value)


def bpmf_gauss_attempts(n_pairs):
    """the attempts of the polar method the device makes at first for n_pairs accepted ones"""
    return int(lib().cmi_bpmf_gauss_attempts(int(n_pairs)))


def bpmf_moments(X, on_device=True):
    """(DenseMatrix.columnMean of every column, DenseMatrix.cov()) of X (rows, k); host-only unless on_device"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    rows, k = X.shape
    mean, cov = np.empty(k), np.empty((k, k))
    _bpmf_chk(lib().cmi_bpmf_moments(_p(X), rows, k, _p(mean), _p(cov), 1 if on_device else 0), "cmi_bpmf_moments")
    return mean, cov


def bpmf_hyper_host(rows, mean, cov, alpha, mu, stream):
    """Host-only: BPMF's hyper-parameter step of one side with `rows` rows; stream = (state, have_cached, cached).
    (alpha, mu, stream after)"""
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    alpha = np.array(alpha, dtype=np.float64, order="C")
    mu = np.array(mu, dtype=np.float64, order="C")
    st, hv, cv = _i64(int(stream[0])), C.c_int(1 if stream[1] else 0), _dbl(float(stream[2]))
    _bpmf_chk(lib().cmi_bpmf_hyper_host(len(mean), int(rows), _p(mean), _p(cov), _p(alpha), _p(mu), C.byref(st), C.byref(hv), C.byref(cv)),
              "cmi_bpmf_hyper_host")
    return alpha, mu, (st.value, bool(hv.value), cv.value)


class BPMFInstance(_FactorModel):
    """The reference's BPMF on one GPU (a `cmi_bpmf_handle`): P is (n_users, k), Q is (n_items, k), 1 <= k <= 64.  P and Q come from the
    caller; the Gibbs and hyper-parameter draws come from the handle's stream (set_stream)."""

    _api = ("cmi_bpmf_create", "cmi_bpmf_destroy", "cmi_bpmf_last_error")
    _prefix = "cmi_bpmf"

    def set_global_mean(self, gm):
        self._chk(self.L.cmi_bpmf_set_global_mean(self.h, float(gm)))

    def global_mean(self):
        gm = _dbl()
        self._chk(self.L.cmi_bpmf_get_global_mean(self.h, C.byref(gm)))
        return gm.value

    def set_model(self, P=None, Q=None):
        P = self._shaped(P, (self.n_users, self.k), "P")
        Q = self._shaped(Q, (self.n_items, self.k), "Q")
        self._chk(self.L.cmi_bpmf_set_model(self.h, None if P is None else _p(P), None if Q is None else _p(Q)))

    def model(self):
        """(P, Q)"""
        P, Q = np.empty((self.n_users, self.k)), np.empty((self.n_items, self.k))
        self._chk(self.L.cmi_bpmf_get_model(self.h, _p(P), _p(Q)))
        return P, Q

    def set_stream(self, state, have_cached=False, cached=0.0):
        self._chk(self.L.cmi_bpmf_set_stream(self.h, int(state), 1 if have_cached else 0, float(cached)))

    def stream(self):
        """(state, have_cached, cached)"""
        st, hv, cv = _i64(), C.c_int(), _dbl()
        self._chk(self.L.cmi_bpmf_get_stream(self.h, C.byref(st), C.byref(hv), C.byref(cv)))
        return st.value, bool(hv.value), cv.value

    def init_hyper(self):
        self._chk(self.L.cmi_bpmf_init_hyper(self.h))

    def hyper(self):
        """(alpha_u, mu_u, alpha_m, mu_m)"""
        k = self.k
        au, mu, am, mm = np.empty((k, k)), np.empty(k), np.empty((k, k)), np.empty(k)
        self._chk(self.L.cmi_bpmf_get_hyper(self.h, _p(au), _p(mu), _p(am), _p(mm)))
        return au, mu, am, mm

    def set_hyper(self, alpha_u, mu_u, alpha_m, mu_m):
        k = self.k
        a = [self._shaped(alpha_u, (k, k), "alpha_u"), self._shaped(mu_u, (k,), "mu_u"), self._shaped(alpha_m, (k, k), "alpha_m"),
             self._shaped(mu_m, (k,), "mu_m")]
        self._chk(self.L.cmi_bpmf_set_hyper(self.h, *[_p(x) for x in a]))

    def iterate(self):
        """one iteration of BPMF.buildModel's loop; returns the loss (a CmiError of code E_NUMERIC carries a non-finite one as .loss)"""
        loss = _dbl()
        rc = self.L.cmi_bpmf_iterate(self.h, C.byref(loss))
        if rc != OK:
            err = CmiError(rc, self.L.cmi_bpmf_last_error(self.h).decode())
            err.loss = loss.value
            raise err
        return loss.value

    def sample_side(self, side, alpha, mu):
        """one Gibbs pass of the users (side 0) or the items (side 1) with the caller's hyper-parameters: (null flags per row, draws)"""
        alpha = self._shaped(alpha, (self.k, self.k), "alpha")
        mu = self._shaped(mu, (self.k,), "mu")
        flags = np.zeros(self.n_users if side == 0 else self.n_items, np.int32)
        draws = _i64()
        self._chk(self.L.cmi_bpmf_sample_side(self.h, int(side), _p(alpha), _p(mu), _p(flags), C.byref(draws)))
        return flags, draws.value

    def predict(self, u, j, bound=False, lo=1.0, hi=5.0):
        u = np.ascontiguousarray(u, dtype=np.int32)
        j = np.ascontiguousarray(j, dtype=np.int32)
        out = np.empty(len(u))
        self._chk(self.L.cmi_bpmf_predict_batch(self.h, len(u), _p(u), _p(j), 1 if bound else 0, float(lo), float(hi), _p(out)))
        return out

    def last_iter_ms(self):
        """(moments, hyper steps on the host, user passes, item passes, loss) milliseconds of the last iterate()"""
        ms = (C.c_float * 5)()
        self._chk(self.L.cmi_bpmf_last_iter_ms(self.h, ms))
        return tuple(ms)
