"""ctypes binding of libsagnn.so (include/sagnn.h). Fails loudly when the library is absent:
the product path has no CPU or eager-PyTorch fallback."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAGNN_LIB points at an alternative build (diagnostic variants under scratch/); default: in-tree
LIB_PATH = os.environ.get("SAGNN_LIB") or os.path.join(_HERE, "lib", "libsagnn.so")


class SagnnError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libsagnn error {code}: {msg}")
        self.code = code


class Tuning(ctypes.Structure):
    _fields_ = [("short_thresh", c_int32), ("long_thresh", c_int32), ("chunk_edges", c_int32),
                ("reserved", c_int32)]


class SpmmEpilogue(ctypes.Structure):
    _fields_ = [("leaky", c_float), ("residual", c_void_p), ("ldr", c_int64), ("out", c_void_p),
                ("ldo", c_int64), ("acc_in", c_void_p), ("ld_acc_in", c_int64), ("acc_out", c_void_p),
                ("ld_acc_out", c_int64), ("mask_out", c_void_p), ("mask_in", c_void_p),
                ("out2", c_void_p), ("ldo2", c_int64), ("slope2", c_float), ("acc_in2", c_void_p),
                ("ld_acc_in2", c_int64)]


class EdgeDropArgs(ctypes.Structure):
    """sagnn_edge_drop"""
    _fields_ = [("seed", c_uint64), ("step", c_uint32), ("keep_threshold", c_uint32), ("scale", c_float)]


class EdgeTimeArgs(ctypes.Structure):
    """sagnn_edge_time"""
    _fields_ = [("te", c_void_p), ("stride_interval", c_int64), ("stride_layer", c_int64), ("stride_dir", c_int64),
                ("n_buckets", c_int32), ("dte", c_void_p), ("adj_user", c_void_p), ("adj_item", c_void_p),
                ("adj_batch", c_void_p), ("adj_workspace", c_void_p), ("adj_workspace_bytes", c_size_t)]


class GnnSide(ctypes.Structure):
    """sagnn_gnn_side"""
    _fields_ = [("in_", c_void_p), ("ld_in", c_int64), ("slab_in", c_int64), ("out", c_void_p), ("ld_out", c_int64),
                ("slab_out", c_int64), ("scratch", c_void_p), ("mask", c_void_p)]


EDGES_PLAIN, EDGES_DROP, EDGES_TIME = 0, 1, 2       # SAGNN_EDGES_*


class GnnArgs(ctypes.Structure):
    """sagnn_gnn_args"""
    _fields_ = [("user", GnnSide), ("item", GnnSide), ("d", c_int), ("n_layers", c_int), ("leaky", c_float),
                ("edges", c_int), ("drop", POINTER(EdgeDropArgs)), ("time", POINTER(EdgeTimeArgs)), ("interval", c_int),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


SOFTMAX_FULL, SOFTMAX_CAND, SOFTMAX_CAND_BIAS = 0, 1, 2       # SAGNN_SOFTMAX_*


class SoftmaxArgs(ctypes.Structure):
    """sagnn_softmax_args"""
    _fields_ = [("Q", c_void_p), ("ldq", c_int64), ("I", c_void_p), ("ldi", c_int64), ("n_queries", c_int64),
                ("n_items", c_int64), ("d", c_int), ("target", c_void_p), ("inv_temp", c_float), ("scale", c_float),
                ("excl_ptr", c_void_p), ("excl_items", c_void_p), ("excl_row", c_void_p), ("n_lists", c_int64),
                ("mode", c_int), ("cand", c_void_p), ("n_cand", c_int64), ("bias", c_void_p), ("loss", c_void_p),
                ("lse", c_void_p), ("tscore", c_void_p), ("g", c_void_p), ("dQ", c_void_p), ("lddq", c_int64),
                ("dI", c_void_p), ("lddi", c_int64), ("dT", c_void_p), ("lddt", c_int64), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t)]


class SeqFfnArgs(ctypes.Structure):
    """sagnn_seq_ffn_args"""
    _fields_ = [("x", c_void_p), ("ldx", c_int64), ("seg_len", c_void_p), ("n_slots", c_int64), ("pos_length", c_int),
                ("d", c_int), ("f", c_int), ("gamma", c_void_p), ("beta", c_void_p), ("ln_eps", c_float), ("W1", c_void_p),
                ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p), ("leaky", c_float)]


class PlanInfo(ctypes.Structure):
    _fields_ = [("n_rows", c_int64), ("n_src", c_int64), ("nnz", c_int64),
                ("n_long_rows", c_int64), ("n_chunks", c_int64), ("short_thresh", c_int32),
                ("long_thresh", c_int32), ("chunk_edges", c_int32), ("max_degree", c_int32),
                ("on_device", c_int32), ("weighted", c_int32)]


# name -> (restype, argtypes); must list every symbol include/sagnn.h declares
SIGNATURES = {
    "sagnn_version": (c_int, []),
    "sagnn_set_engine": (c_int, [c_int]),
    "sagnn_get_engine": (c_int, []),
    "sagnn_range_redo_count": (c_int, [POINTER(c_int64), c_int]),
    "sagnn_last_error": (c_size_t, [c_char_p, c_size_t]),
    "sagnn_profile_enable": (c_int, [c_int]),
    "sagnn_profile_read": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, POINTER(c_int)]),
    "sagnn_csr_check_host": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "sagnn_spmm_plan_create": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                       POINTER(Tuning), POINTER(c_void_p)]),
    "sagnn_spmm_plan_destroy": (c_int, [c_void_p]),
    "sagnn_spmm_plan_get_info": (c_int, [c_void_p, POINTER(PlanInfo)]),
    "sagnn_spmm_plan_set_weights": (c_int, [c_void_p, c_void_p]),
    "sagnn_spmm_plan_copy_chunks": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "sagnn_spmm_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "sagnn_spmm_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float,
                               c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                               c_size_t, c_void_p]),
    "sagnn_spmm_ex_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(SpmmEpilogue), c_void_p, c_size_t,
                                  c_void_p]),
    "sagnn_mask_scale_f32": (c_int, [c_void_p, c_int64, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "sagnn_spmm_batch_create": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_void_p)]),
    "sagnn_spmm_batch_destroy": (c_int, [c_void_p]),
    "sagnn_spmm_batch_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "sagnn_gnn_interval_f32": (c_int, [c_void_p, c_void_p, POINTER(GnnArgs), c_void_p]),
    "sagnn_gnn_interval_bwd_f32": (c_int, [c_void_p, c_void_p, POINTER(GnnArgs), c_void_p]),
    "sagnn_gnn_stack_f32": (c_int, [c_void_p, POINTER(GnnArgs), c_void_p]),
    "sagnn_gnn_stack_bwd_f32": (c_int, [c_void_p, POINTER(GnnArgs), c_void_p]),
    "sagnn_spmm_drop_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(SpmmEpilogue), POINTER(EdgeDropArgs),
                                    c_uint32, c_int, c_void_p, c_size_t, c_void_p]),
    "sagnn_spmm_plan_set_buckets": (c_int, [c_void_p, c_void_p, c_int32]),
    "sagnn_spmm_time_batch_create": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_void_p)]),
    "sagnn_spmm_time_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, POINTER(SpmmEpilogue), POINTER(EdgeDropArgs),
                                    POINTER(EdgeTimeArgs), c_void_p, c_size_t, c_void_p]),
    "sagnn_lstm_fwd_train_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_float,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sagnn_mhsa_wide_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sagnn_ln_mhsa_mean_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "sagnn_ln_mhsa_mean_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p,
                                       c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p, c_size_t, c_void_p]),
    "sagnn_mhsa_mean_wide_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_size_t,
                                         c_void_p]),
    "sagnn_attn_bwd_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "sagnn_layernorm_td_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p,
                                           c_float, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sagnn_lstm_bwd_step_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "sagnn_attn_bwd_front_supported": (c_int, [c_int, c_int, c_int]),
    "sagnn_attn_bwd_front_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p,
                                         c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sagnn_attn_bwd_tail_supported": (c_int, [c_int]),
    "sagnn_attn_bwd_tail_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sagnn_lstm_bwd_supported": (c_int, [c_int]),
    "sagnn_lstm_bwd_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "sagnn_lstm_bwd_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sagnn_lstm_bwd_ws_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "sagnn_gru_fused_supported": (c_int, [c_int]),
    "sagnn_gru_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sagnn_gru_fwd_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sagnn_gru_bwd_cand_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                       c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "sagnn_gru_bwd_gates_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                        c_int, c_int, c_int, c_void_p]),
    "sagnn_leaky_add_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "sagnn_pair_score_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                     c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_pair_score_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_prod_leaky_sum_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p,
                                         c_int64, c_int, c_void_p]),
    "sagnn_prod_leaky_sum_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float,
                                             c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_meta_features_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                        c_void_p]),
    "sagnn_meta_features_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_leaky_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int, c_void_p]),
    "sagnn_rowdot_sigmoid_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_rowdot_sigmoid_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                             c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "sagnn_hinge_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sagnn_mul_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sagnn_adam_step_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float,
                                    c_float, c_float, c_int64, c_void_p]),
    "sagnn_adam_multi_f32": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float,
                                     c_float, c_float, c_int64, c_void_p]),
    "sagnn_dense_nn_f32": (c_int, [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                   c_int, c_void_p]),
    "sagnn_dense_tn_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p]),
    "sagnn_dense_tn_seg_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p]),
    "sagnn_lstm_fwd_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p,
                                   c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "sagnn_lstm_fwd_state_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_float,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "sagnn_layernorm_td_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p,
                                       c_float, c_void_p, c_int64, c_void_p]),
    "sagnn_mhsa_mean_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_void_p]),
    "sagnn_interval_fusion_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_float, c_void_p, c_void_p, c_float, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int64, c_void_p, c_size_t, c_void_p]),
    "sagnn_interval_fusion_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "sagnn_score_topk_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int, c_int]),
    "sagnn_score_topk_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sagnn_candidate_rank_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                         c_void_p, c_void_p, c_int64, c_void_p, c_float, c_int64, c_int, c_int, c_void_p,
                                         c_void_p, c_int64, c_void_p]),
    "sagnn_sample_train_i32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                       c_int, c_int, c_int, c_void_p, c_int64, c_uint64, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "sagnn_sample_ssl_i32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                     c_uint64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sagnn_seq_sum_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_sum_bwd_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                      c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "sagnn_rows_mark_i32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sagnn_rows_mark_seg_i32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "sagnn_rows_compact_workspace_bytes": (c_size_t, [c_int64]),
    "sagnn_rows_compact_i32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sagnn_rows_gather_f32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p,
                                      c_void_p, c_void_p]),
    "sagnn_rows_scatter_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_void_p, c_int64, c_int64,
                                       c_int64, c_void_p]),
    "sagnn_seq_attn_supported": (c_int, [c_int, c_int, c_int]),
    "sagnn_seq_gather_f32": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p,
                                     c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_gather_bwd_f32": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                         c_int64, c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_attn_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sagnn_seq_attn_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sagnn_seq_pool_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_pool_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_attn_masked_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sagnn_seq_attn_masked_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p,
                                              c_void_p]),
    "sagnn_seq_attn_wide_supported": (c_int, [c_int, c_int, c_int]),
    "sagnn_seq_attn_wide_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "sagnn_seq_attn_wide_bwd_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p]),
    "sagnn_seq_ffn_supported": (c_int, [c_int, c_int, c_int]),
    "sagnn_seq_ffn_f32": (c_int, [POINTER(SeqFfnArgs), c_void_p, c_int64, c_void_p]),
    "sagnn_seq_ffn_bwd_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "sagnn_seq_ffn_bwd_f32": (c_int, [POINTER(SeqFfnArgs), c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "sagnn_seq_prefix_query_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_float,
                                           c_void_p, c_int64, c_void_p]),
    "sagnn_seq_prefix_query_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_float,
                                               c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "sagnn_seq_targets_i32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64,
                                      c_void_p, c_void_p, c_void_p]),
    "sagnn_softmax_target_scatter_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64,
                                                 c_void_p]),
    "sagnn_seq_addpool_supported": (c_int, [c_int, c_int, c_int]),
    "sagnn_seq_addpool_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                      c_void_p, c_int64, c_void_p, c_void_p]),
    "sagnn_seq_addpool_bwd_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                          c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                          c_void_p]),
    "sagnn_softmax_loss_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "sagnn_softmax_loss_f32": (c_int, [POINTER(SoftmaxArgs), c_void_p]),
    "sagnn_softmax_loss_bwd_f32": (c_int, [POINTER(SoftmaxArgs), c_void_p]),
    "sagnn_sample_strata_i32": (c_int, [c_int64, c_int64, c_uint64, c_uint32, c_void_p, c_void_p]),
    "sagnn_softmax_target_add_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "sagnn_softmax_loss_cand_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "sagnn_sample_strata_w_i32": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_uint64, c_uint32, c_void_p, c_void_p,
                                          c_void_p]),
    "sagnn_softmax_cand_scatter_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p,
                                               c_int64, c_void_p]),
}


_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C sa-gnn_amd/csrc`). There is no fallback path.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.sagnn_version.restype = c_int
    if lib.sagnn_version() < 10500:     # before 1.5.0 the softmax-loss entries took positional arguments under the same names
        raise ImportError(f"{LIB_PATH} is libsagnn {lib.sagnn_version()}: this binding needs >= 10500 (sagnn_softmax_args)")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    buf = ctypes.create_string_buffer(1024)
    load().sagnn_last_error(buf, 1024)
    return buf.value.decode("utf-8", "replace")


def check(rc: int) -> None:
    if rc != 0:
        raise SagnnError(rc, last_error())
