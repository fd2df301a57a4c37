"""ctypes binding of libstemgnn_hip.so (C ABI declared in include/stemgnn_hip.h).

Fails loudly: a missing / unloadable library raises at first use -- there is no fallback path.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_ulonglong, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STEMGNN_HIP_LIB", os.path.join(_HERE, "libstemgnn_hip.so"))   # override: A/B builds only
SG_BLOCK_NPARAMS = 33
SG_EINVAL = -10001
SG_LOSS = {"mse": 0, "mae": 1, "huber": 2}    # SG_LOSS_* in include/stemgnn_hip.h
SG_SCENARIO_COUPLING = {"independent": 0, "path": 1}    # SG_SCENARIO_* in include/stemgnn_hip.h
SG_SCENARIO_TAILS = {"linear": 0, "clamp": 1}
SG_LOSS_PINBALL = 3                           # the quantile head's loss: its own `_quantile` entries, not a `_loss` kind
# bits of stemgnn_block_paths (SG_PATH_* in include/stemgnn_hip.h)
SG_PATH = {"glu_fwd_fused": 1, "glu_dgrad_fused": 2, "heads_fwd_fused": 4, "heads_bwd_fused": 8, "heads_bwd_16w": 16,
           "long_k": 32, "wgrad_fused": 64, "glu_wgrad_fused": 128}
# words of stemgnn_gru_paths (SG_GRU_* in include/stemgnn_hip.h), the kernel families and the dW_hh forms
SG_GRU_PATH_WORDS = 16
SG_GRU_WORD = {"fwd_family": 0, "fwd_P": 1, "fwd_K": 2, "gi_stream": 3, "bwd_family": 4, "bwd_P": 5, "bwd_KU": 6,
               "bwd_slices": 7, "ih_folded": 8, "hh_form": 9, "ih_slabs": 10, "rank2_ok": 11, "wide_passes": 12,
               "wide_MT": 13, "wide_GWf": 14, "wide_GWb": 15}
SG_GRU_FAM = {"stream": 0, "cluster1": 1, "cluster2": 2, "cluster4": 3, "wide": 4}
SG_GRU_HH = {"slabs": 0, "tiles": 1, "flat": 2}


def gru_paths(B, S, Hd, W, cus=0):
    """stemgnn_gru_paths as a dict of SG_GRU_WORD names (cus = 0: the current device); raises on SG_EINVAL."""
    out = (c_int * SG_GRU_PATH_WORDS)()
    check(load().stemgnn_gru_paths(B, S, Hd, W, cus, out), "stemgnn_gru_paths")
    return {k: int(out[i]) for k, i in SG_GRU_WORD.items()}


# words of one kernel family in stemgnn_fc_tail_plan (include/stemgnn_hip.h): 12 for the 64-row entries, then 12 for the training ones
SG_TAIL_PLAN_WORDS = 24
SG_TAIL_WORD = {"rows": 0, "row_threads": 1, "nblocks": 2, "nacc": 3, "slots": 4, "reduce_grid": 5, "reduce_lanes": 6,
                "reduce_trip": 7, "lds0": 8, "lds0_raised": 9, "lds1": 10, "lds1_raised": 11}


def fc_tail_plan(B, N, W, H):
    """stemgnn_fc_tail_plan as {"plain": {...}, "train": {...}} of SG_TAIL_WORD names; raises on SG_EINVAL."""
    out = (c_int * SG_TAIL_PLAN_WORDS)()
    check(load().stemgnn_fc_tail_plan(B, N, W, H, out), "stemgnn_fc_tail_plan")
    return {fam: {k: int(out[12 * f + i]) for k, i in SG_TAIL_WORD.items()} for f, fam in enumerate(("plain", "train"))}


# entries and words of stemgnn_data_plan (SG_DATA_* in include/stemgnn_hip.h)
SG_DATA_ENTRY = {"normalize": 0, "gather": 1, "gather_queue": 2, "mse_fwd": 3, "mse_bwd": 4, "roll": 5, "roll_quantile": 6,
                 "forecast_store": 7, "eval": 8, "quantile_metrics": 9}
SG_DATA_PLAN_WORDS = 9
SG_DATA_WORD = {"grid_x": 0, "grid_y": 1, "grid_z": 2, "threads": 3, "vec": 4, "rows_per_wg": 5, "form": 6, "passes": 7,
                "nchunk": 8}


def data_plan(entry, *shape):
    """stemgnn_data_plan as a dict of SG_DATA_WORD names; `entry` a key of SG_DATA_ENTRY, `shape` as the header lists it for that
    entry; raises on SG_EINVAL."""
    out = (c_int * SG_DATA_PLAN_WORDS)()
    args = list(shape) + [0] * (5 - len(shape))
    check(load().stemgnn_data_plan(SG_DATA_ENTRY[entry], *args, out), f"stemgnn_data_plan({entry}, {shape})")
    return {k: int(out[i]) for k, i in SG_DATA_WORD.items()}


# entries and words of stemgnn_serving_plan (SG_SERVING_* in include/stemgnn_hip.h): the common words, then each entry's own
SG_SERVING_ENTRY = {"push": 0, "gather": 1, "aci": 2, "anomaly": 3}
SG_SERVING_FORM = {"columns": 0, "stream": 1, "pooled": 2}
SG_SERVING_PLAN_WORDS = 22
SG_SERVING_WORD = {"form": 0, "grid_x": 1, "grid_y": 2, "grid_z": 3, "threads": 4, "vec": 5, "launches": 6}
SG_SERVING_ENTRY_WORD = {
    "push": {"k0": 7},
    "gather": {"trips": 7},
    "aci": {"Cc": 7, "Hr": 8, "L": 9, "G": 10, "wd_last": 11, "keep": 12, "step_full": 13, "step_last": 14, "pass_trips_full": 15,
            "pass_trips_last": 16, "origin_trips_full": 17, "origin_trips_last": 18, "tile": 19},
    "anomaly": {"hspan": 7, "spans": 8, "rparts": 9, "tiles": 10, "pop_trips": 11, "want": 12, "most": 13, "parts": 14,
                "batches": 15, "nb_last": 16, "p2_last": 17, "L": 18, "G": 19, "tile": 20,
                "row_lanes": 21},
}


def serving_plan(entry, *shape, misaligned=0):
    """stemgnn_serving_plan as a dict of SG_SERVING_WORD and the entry's SG_SERVING_ENTRY_WORD names; `entry` a key of
    SG_SERVING_ENTRY, `shape` as the header lists it for that entry, `misaligned` its bit set; raises on SG_EINVAL."""
    out = (c_int * SG_SERVING_PLAN_WORDS)()
    args = [int(v) for v in shape] + [0] * (6 - len(shape))
    check(load().stemgnn_serving_plan(SG_SERVING_ENTRY[entry], *args, int(misaligned), out),
          f"stemgnn_serving_plan({entry}, {shape}, {misaligned})")
    return {k: int(out[i]) for k, i in {**SG_SERVING_WORD, **SG_SERVING_ENTRY_WORD[entry]}.items()}


# entries and words of stemgnn_calibration_plan (SG_CALIBRATION_* in include/stemgnn_hip.h): the common words, then each entry's own
SG_CALIBRATION_ENTRY = {"fit": 0, "seasonal_fit": 1, "apply": 2, "seasonal_apply": 3, "column": 4}
SG_CALIBRATION_NSHAPE = {"fit": 6, "seasonal_fit": 9, "apply": 4, "seasonal_apply": 4, "column": 6}
SG_CALIBRATION_FORM = {"columns": 0, "stream": 1}
SG_CALIBRATION_BOUND = {"wanted": 0, "size": 1, "grid": 2}
SG_CALIBRATION_WALK = {"direct": 0, "origins": 1, "one_bucket": 2, "long": 3}
SG_CALIBRATION_PLAN_WORDS = 32
SG_CALIBRATION_WORD = {"form": 0, "grid_x": 1, "grid_y": 2, "grid_z": 3, "threads": 4, "vec": 5, "cus": 6}
_FIT_WORDS = {"KP": 7, "groups": 8, "Cc": 9, "Hr": 10, "L": 11, "G": 12, "tiles": 13, "wd_last": 14, "rpw_full": 15, "rpw_last": 16,
              "tile": 17, "chunks": 18, "per_chunk": 19, "bound": 20, "trips": 21, "want": 22, "by_size": 23, "blocks_wanted": 24,
              "pick_blocks": 25, "pick_idle": 26, "rows": 27, "direct": 28, "why": 29, "runs": 30, "walk": 31}
_APPLY_WORDS = {"needed": 7, "cap": 8, "capped": 9, "trips": 10, "lane_trips": 11, "items": 12}
SG_CALIBRATION_ENTRY_WORD = {
    "fit": _FIT_WORDS, "seasonal_fit": _FIT_WORDS, "apply": _APPLY_WORDS, "seasonal_apply": _APPLY_WORDS,
    "column": {"lds": 7, "planes": 8, "cpb": 9, "wpb": 10, "idle": 11, "col_blocks": 12, "cols_last": 13, "win_blocks": 14,
               "capped": 15, "win_trips": 16, "tvec": 17, "target_trips": 18, "per": 19},
}


def calibration_plan(entry, *shape, misaligned=0):
    """stemgnn_calibration_plan as a dict of SG_CALIBRATION_WORD and the entry's SG_CALIBRATION_ENTRY_WORD names; `entry` a key of
    SG_CALIBRATION_ENTRY, `shape` as the header lists it for that entry, `misaligned` its bit set; raises on SG_EINVAL."""
    out = (c_int * SG_CALIBRATION_PLAN_WORDS)()
    args = (c_long * len(shape))(*[int(v) for v in shape])
    check(load().stemgnn_calibration_plan(SG_CALIBRATION_ENTRY[entry], args, len(shape), int(misaligned), out),
          f"stemgnn_calibration_plan({entry}, {shape}, {misaligned})")
    return {k: int(out[i]) for k, i in {**SG_CALIBRATION_WORD, **SG_CALIBRATION_ENTRY_WORD[entry]}.items()}


_P = c_void_p          # device pointer
_PP = POINTER(c_void_p)  # host array of device pointers

# name -> (restype, argtypes); mirrors include/stemgnn_hip.h one to one
SIGNATURES = {
    "stemgnn_version": (c_char_p, []),
    "stemgnn_num_cus": (c_int, []),
    "stemgnn_table_floats": (c_size_t, [c_int, c_int]),
    "stemgnn_packed_floats": (c_size_t, [c_int, c_int]),
    "stemgnn_saved_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_scratch_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_scratch_offset_dG": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_gradpart_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_attn_saved_floats": (c_size_t, [c_int, c_int]),
    "stemgnn_attn_scratch_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_make_tables_host": (c_int, [c_int, c_int, _P]),
    "stemgnn_attn_laplacian_fwd": (c_int, [_P, _P, _P, c_float, c_float, c_int, _P, c_int, c_int, _P, _P, _P, c_int, _P]),
    "stemgnn_attn_laplacian_bwd": (c_int, [_P, _P, _P, _P, c_float, c_float, c_int, _P, c_int, c_int, _P, _P, c_int,
                                           _P, _P, _P, c_int, _P]),
    "stemgnn_attn_laplacian_bwd_ext": (c_int, [_P, _P, _P, _P, _P, c_float, c_float, c_int, _P, c_int, c_int, _P, _P, c_int,
                                               _P, _P, _P, c_int, _P]),
    "stemgnn_dropout_mask": (c_int, [c_float, _P, c_int, c_int, _P, _P]),
    "stemgnn_dropout_seed_next": (c_int, [_P, _P, _P]),
    "stemgnn_cheb_fwd": (c_int, [_P, c_int, _P]),
    "stemgnn_cheb_bwd": (c_int, [_P, _P, _P, _P, c_int, _P]),
    "stemgnn_graph_degree": (c_int, [_P, c_int, _P, _P]),
    "stemgnn_graph_basis_fwd": (c_int, [_P, _P, _P, _P, c_int, _P]),
    "stemgnn_graph_basis_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, _P]),
    "stemgnn_graph_accumulate": (c_int, [_P, c_double, _P, c_size_t, c_int, _P]),
    "stemgnn_graph_finish": (c_int, [_P, c_double, _P, c_size_t, _P]),
    "stemgnn_eigh_scratch_floats": (c_size_t, [c_int]),
    "stemgnn_eigh_fwd": (c_int, [_P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_eigh_batched": (c_int, [_P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_eigh_status": (c_int, []),
    "stemgnn_eigh_cluster_fixes": (c_int, []),
    "stemgnn_split_planes_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_split_weights_bf16": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "stemgnn_glu_gemm_bf16": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_glu_gemm_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "stemgnn_sgemm_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_sgemm_paths": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_glu_combine_fwd": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_glu_combine_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_colsum": (c_int, [_P, c_int, c_int, _P, _P]),
    "stemgnn_glu_fused_repack": (c_int, [_P, c_int, c_int, _P]),
    "stemgnn_shortcut_dx": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_gru_reserve_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_gru_fwd_scratch_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_gru_bwd_scratch_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_gru_bwd_cus": (c_int, [c_int, c_int]),
    "stemgnn_gru_paths": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int)]),
    "stemgnn_gru_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd_rank2_ok": (c_int, [c_int, c_int]),
    "stemgnn_gru_bwd_rank2": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd_rank2_dq": (c_int, [_P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd_overlap_ok": (c_int, [c_int, c_int, c_int, c_int]),
    "stemgnn_gru_bwd_ctl_words": (c_size_t, [c_int]),
    "stemgnn_gru_bwd_rank2_begin": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd_rank2_finish": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_gru_bwd_recur": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "stemgnn_gru_bwd_rank2_recur": (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "stemgnn_gru_input_grad": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "stemgnn_keyquery_wgrad": (c_int, [_P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_attn_dquery_reduce": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "stemgnn_keyquery_wgrad2": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, _P]),
    "stemgnn_fc_tail_supported": (c_int, [c_int, c_int]),
    "stemgnn_fc_tail_scratch_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_fc_tail_plan": (c_int, [c_int, c_int, c_int, c_int, _P]),
    "stemgnn_fc_tail_fwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "stemgnn_fc_tail_bwd": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_fill_zero": (c_int, [_P, c_size_t, _P]),
    "stemgnn_rmsprop_step": (c_int, [_P, _P, _P, c_size_t, _P, c_float, c_float, c_int, c_float, _P]),
    "stemgnn_adam_step": (c_int, [_P, _P, _P, _P, c_size_t, _P, _P, c_float, c_float, c_float, c_int, c_float, _P]),
    "stemgnn_grad_norm_partials": (c_size_t, [c_size_t]),
    "stemgnn_grad_sqsum": (c_int, [_P, c_size_t, c_float, _P, _P]),
    "stemgnn_rmsprop_step_ext": (c_int, [_P, _P, _P, c_size_t, _P, c_float, c_float, c_int, c_float, c_float, c_float, c_int,
                                         _P, _P, _P]),
    "stemgnn_adam_step_ext": (c_int, [_P, _P, _P, _P, c_size_t, _P, _P, c_float, c_float, c_float, c_int, c_float, c_float,
                                      c_int, c_float, c_int, _P, _P, _P]),
    "stemgnn_normalize_series": (c_int, [_P, _P, _P, c_int, _P, c_long, c_int, _P]),
    "stemgnn_window_gather": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_long, _P, _P]),
    "stemgnn_window_gather_queue": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_long, _P, _P]),
    "stemgnn_window_gather_pair": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_long, _P, _P]),
    "stemgnn_window_gather_queue_pair": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_long, _P, _P]),
    "stemgnn_mse_scratch_floats": (c_size_t, []),
    "stemgnn_mse_fwd": (c_int, [_P, _P, c_size_t, _P, _P, _P, _P]),
    "stemgnn_mse_bwd": (c_int, [_P, _P, c_size_t, _P, _P, _P]),
    "stemgnn_roll_window": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_forecast_store": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_long, _P]),
    "stemgnn_eval_scratch_doubles": (c_size_t, [c_long, c_int, c_int]),
    "stemgnn_eval_out_doubles": (c_size_t, [c_int, c_int]),
    "stemgnn_eval_metrics": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, _P, _P, _P]),
    "stemgnn_eval_scratch_doubles_masked": (c_size_t, [c_long, c_int, c_int]),
    "stemgnn_eval_metrics_masked": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, _P, _P, _P]),
    "stemgnn_data_plan": (c_int, [c_int, c_long, c_long, c_long, c_long, c_long, POINTER(c_int)]),
    "stemgnn_block_pack": (c_int, [_PP, _P, _P, c_int, c_int, _P]),
    "stemgnn_block_pack_panels": (c_int, [_PP, _P, _P, c_int, c_int, _P]),
    "stemgnn_block_unpack_grads": (c_int, [_P, c_int, _P, _PP, c_int, c_int, c_int, _P]),
    "stemgnn_gft_fwd": (c_int, [_P, _P, c_long, c_long, c_long, _P, c_int, c_int, c_int, _P]),
    "stemgnn_gft_bwd": (c_int, [_P, _P, c_long, c_long, c_long, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_gft_bwd_dt2": (c_int, [_P, c_long, c_long, c_long, _P, _P, c_long, c_long, c_long, _P, _P, c_int, c_int, c_int, _P]),
    "stemgnn_spectral_glu_fwd": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_spectral_glu_bwd": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_glu_split_floats": (c_size_t, [c_int, c_int, c_int]),
    "stemgnn_glu_split_panels": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "stemgnn_glu_fused_bf16_ok": (c_int, [c_int, c_int, c_int]),
    "stemgnn_block_paths": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "stemgnn_spectral_glu_fwd_split": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_glu_warm_saved_floats": (c_size_t, [c_int, c_int]),
    "stemgnn_spectral_glu_fwd_warm": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_spectral_glu_dgrad_split": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_igft_heads_fwd": (c_int, [_PP, _P, _P, _P, c_long, c_long, c_long, _P, c_int, _P,
                                       c_int, c_int, c_int, c_int, _P]),
    "stemgnn_igft_heads_bwd": (c_int, [_PP, _P, _P, _P, c_long, c_long, c_long, _P, _P, _P, _P, _P, c_int, c_int,
                                       c_int, c_int, c_int, c_int, _P]),
    "stemgnn_fc_tail_train_scratch_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_fc_tail_train": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P,
                                      _P, _P]),
    "stemgnn_fc_tail_train_rows": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_fc_tail_train_finish": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_target_valid_count": (c_int, [_P, c_size_t, _P, _P]),
    "stemgnn_fc_tail_train_loss": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P,
                                           _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_fc_tail_train_rows_loss": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, _P,
                                                _P, _P]),
    "stemgnn_fc_tail_train_finish_loss": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_fc_tail_train_quantile": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), _P,
                                               _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_fc_tail_train_rows_quantile": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float),
                                                    _P, _P, _P, _P, _P]),
    "stemgnn_fc_tail_train_finish_quantile": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "stemgnn_roll_window_quantile": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_quantile_scratch_doubles": (c_size_t, [c_long, c_int, c_int, c_int]),
    "stemgnn_quantile_out_doubles": (c_size_t, [c_int, c_int]),
    "stemgnn_quantile_metrics": (c_int, [_P, _P, POINTER(c_double), _P, _P, c_long, c_int, c_int, c_int, _P, _P, _P]),
    "stemgnn_quantile_metrics_masked": (c_int, [_P, _P, POINTER(c_double), _P, _P, c_long, c_int, c_int, c_int, _P, _P, _P]),
    "stemgnn_conformal_rank": (c_long, [c_long, c_double]),
    "stemgnn_conformal_scratch_bytes": (c_size_t, [c_long, c_int, c_int, c_int, c_int, c_int]),
    "stemgnn_conformal_fit": (c_int, [_P, _P, c_long, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int),
                                      POINTER(c_double), c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_conformal_apply": (c_int, [_P, _P, c_long, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), c_int,
                                        c_int, _P, _P]),
    "stemgnn_quantile_finish": (c_int, [_P, c_long, c_int, c_int, c_int, c_int, _P, c_int, POINTER(c_int), POINTER(c_int),
                                        c_int, c_int, _P, _P]),
    "stemgnn_quantile_store": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, POINTER(c_int),
                                       POINTER(c_int), c_int, c_int, _P, _P, c_long, _P]),
    "stemgnn_season_bucket": (c_int, [c_longlong, c_longlong, c_int, c_longlong]),
    "stemgnn_seasonal_scratch_bytes": (c_size_t, [c_long, c_int, c_int, c_int, c_int, c_int, c_int]),
    "stemgnn_seasonal_fit": (c_int, [_P, _P, _P, c_longlong, c_long, c_int, c_int, c_int, c_int, POINTER(c_int),
                                     POINTER(c_int), POINTER(c_double), c_int, c_int, c_int, c_longlong, c_int, c_longlong,
                                     _P, _P, _P, _P]),
    "stemgnn_seasonal_apply": (c_int, [_P, _P, _P, c_longlong, c_long, c_int, c_int, c_int, c_int, c_int, POINTER(c_int),
                                       POINTER(c_int), c_int, c_int, c_longlong, c_int, c_longlong, _P, _P]),
    "stemgnn_quantile_store_seasonal": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, POINTER(c_int),
                                                POINTER(c_int), c_int, c_int, c_longlong, c_int, c_longlong, _P, _P, c_long,
                                                _P]),
    "stemgnn_live_push": (c_int, [_P, c_int, c_int, c_longlong, _P, _P, c_int, c_double, c_int, _P, _P, _P, c_int, _P, _P]),
    "stemgnn_ring_gather": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "stemgnn_live_head": (c_int, [_P, c_long, _P, _P, _P]),
    "stemgnn_aci_update": (c_int, [_P, _P, _P, c_int, c_longlong, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int),
                                   POINTER(c_double), c_double, c_int, c_int, c_longlong, c_int, c_int, _P, _P, _P, _P, _P, _P,
                                   _P]),
    "stemgnn_anomaly_update": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_longlong, _P, c_int, c_int, c_int, c_int, c_int,
                                       c_longlong, c_double, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P,
                                       _P]),
    "stemgnn_serving_plan": (c_int, [c_int, c_long, c_long, c_long, c_long, c_long, c_long, c_int, POINTER(c_int)]),
    "stemgnn_calibration_plan": (c_int, [c_int, POINTER(c_long), c_int, c_int, POINTER(c_int)]),
    "stemgnn_scenario_rank": (c_long, [c_double, c_long]),
    "stemgnn_scenario_roll": (c_int, [_P, _P, POINTER(c_float), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_longlong, c_ulonglong, c_ulonglong, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_scenario_bands": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_int, _P, _P]),
    "stemgnn_scenario_roll_given": (c_int, [_P, _P, POINTER(c_float), _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_copula_pit": (c_int, [_P, _P, POINTER(c_float), c_long, c_int, c_int, c_int, c_int, _P, _P]),
    "stemgnn_copula_scratch_doubles": (c_size_t, [c_long, c_int]),
    "stemgnn_copula_gram": (c_int, [_P, c_long, c_int, _P, _P, _P, _P]),
    "stemgnn_copula_uniforms": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_longlong, c_ulonglong, c_ulonglong, _P,
                                        _P]),
    "stemgnn_copula_uniforms_steps": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_longlong, c_ulonglong,
                                              c_ulonglong, _P, _P]),
    "stemgnn_ensemble_scratch_doubles": (c_size_t, [c_long, c_int, c_int, c_int]),
    "stemgnn_ensemble_out_doubles": (c_size_t, [c_int]),
    "stemgnn_ensemble_scores": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_ensemble_scores_masked": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_scenario_aggregate": (c_int, [_P, _P, _P, _P, c_longlong, c_int, c_int, _P, _P]),
    "stemgnn_scenario_events": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "stemgnn_scenario_distances": (c_int, [_P, _P, c_long, c_int, c_int, c_int, _P, _P]),
    "stemgnn_scenario_reduce": (c_int, [_P, c_long, c_int, c_int, _P, _P, _P, _P, _P]),
    "stemgnn_weighted_bands": (c_int, [_P, _P, c_long, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), _P, _P]),
    "stemgnn_weighted_scratch_doubles": (c_size_t, [c_long, c_int, c_int, c_int]),
    "stemgnn_weighted_out_doubles": (c_size_t, [c_int]),
    "stemgnn_weighted_scores": (c_int, [_P, _P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_weighted_events": (c_int, [_P, _P, _P, _P, _P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "stemgnn_scenario_reduce_weighted": (c_int, [_P, _P, c_long, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "stemgnn_scenario_stage_distances": (c_int, [_P, _P, c_long, c_int, c_int, c_int, c_int, POINTER(c_int), c_int, _P, _P]),
    "stemgnn_scenario_tree": (c_int, [_P, _P, c_long, c_int, c_int, POINTER(c_int), c_int, _P, _P, _P, _P, _P, _P]),
    "stemgnn_scenario_envelope": (c_int, [_P, _P, c_int, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_double, _P, _P, _P,
                                          _P, _P, _P]),
    "stemgnn_infer_workspace_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "stemgnn_infer_workspace_split_floats": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "stemgnn_gru_fwd_infer": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "stemgnn_spectral_glu_fwd_infer": (c_int, [_P, _P, c_size_t, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_spectral_glu_fwd_split_infer": (c_int, [_P, _P, _P, c_size_t, c_int, c_int, c_int, c_int, c_int, _P]),
    "stemgnn_igft_heads_fwd_infer": (c_int, [_PP, _P, _P, c_size_t, _P, c_long, c_long, c_long, _P, c_int, _P,
                                             c_int, c_int, c_int, c_int, _P]),
    "stemgnn_block_wgrad": (c_int, [_PP, _P, _P, _P, c_long, c_long, c_long, _P, c_int, _P, _P, c_int, c_int,
                                    c_int, c_int, c_int, c_int, _P]),
    "stemgnn_block_wgrad_split": (c_int, [_PP, _P, _P, _P, c_long, c_long, c_long, _P, c_int, _P, _P, c_int, c_int,
                                          c_int, c_int, c_int, c_int, c_int, _P]),
}

_lib = None


class StemGNNHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise StemGNNHipError(
            f"{LIB_PATH} not found -- build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950); "
            "stemgnn_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        if rc == SG_EINVAL:
            raise StemGNNHipError(f"{what}: invalid argument (SG_EINVAL)")
        raise StemGNNHipError(f"{what}: HIP error {-rc}")


def host_floats(values, ctype=c_float):
    """host array of the quantile levels (`taus` of the `_quantile` entries: read by the call itself, in host memory)."""
    return (ctype * len(values))(*[float(v) for v in values])


def ptr_array(tensors):
    """host array of SG_BLOCK_NPARAMS device pointers (None -> NULL)."""
    arr = (c_void_p * SG_BLOCK_NPARAMS)()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr
