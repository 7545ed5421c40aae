"""ctypes binding of libtfgnn.so (the C ABI declared in include/tfgnn.h).

There is deliberately NO fallback: if the HIP library has not been built (``python -m
tf2_gnn_amd.build``) or cannot be loaded, every op raises ``RuntimeError``.  PyTorch is used for
device allocation and the current HIP stream only.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libtfgnn.so"

# (name, restype, argtypes) - one row per symbol declared in include/tfgnn.h
_SIGNATURES = [
    ("tfgnn_last_error", c_char_p, []),
    ("tfgnn_version", c_char_p, []),
    ("tfgnn_abi_version", c_int, []),
    ("tfgnn_gemm_gathered_supported", c_int, [c_int64, c_int64, c_int64, c_int64, c_int64]),
    ("tfgnn_launch_counts", c_int, [POINTER(c_int64), c_int]),
    ("tfgnn_sp_spread_flag", c_int, [c_int]),
    ("tfgnn_sp_guard_repair", c_int, [c_int]),
    ("tfgnn_sp_repair_stats", c_int, [POINTER(c_int64), c_int]),
    (
        "tfgnn_graph_create",
        c_int,
        [c_int, c_int64, POINTER(c_void_p), POINTER(c_int64), c_void_p, POINTER(c_void_p)],
    ),
    ("tfgnn_graph_destroy", c_int, [c_void_p]),
    (
        "tfgnn_graph_create_async",
        c_int,
        [c_int, c_int64, POINTER(c_void_p), POINTER(c_int64), c_void_p, POINTER(c_void_p)],
    ),
    ("tfgnn_graph_wait", c_int, [c_void_p]),
    (
        "tfgnn_graph_create_parts_async",
        c_int,
        [c_int, c_int64, POINTER(c_void_p), POINTER(c_int64), ctypes.c_uint, c_void_p, POINTER(c_void_p)],
    ),
    ("tfgnn_graph_ensure", c_int, [c_void_p, ctypes.c_uint, c_void_p]),
    ("tfgnn_graph_parts", ctypes.c_uint, [c_void_p]),
    ("tfgnn_graph_destroy_async", c_int, [c_void_p, c_void_p]),
    ("tfgnn_graph_array", c_int, [c_void_p, c_int, POINTER(c_void_p), POINTER(c_int64)]),
    ("tfgnn_graph_dims", c_int, [c_void_p, POINTER(c_int64), POINTER(c_int), POINTER(c_int64)]),
    ("tfgnn_graph_scales", c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_graph_target_multiplier", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    (
        "tfgnn_csr_gather_reduce",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
         c_int, c_int, c_int, c_void_p],
    ),
    ("tfgnn_graph_gather_workspace_bytes", c_size_t, [c_void_p, c_int, c_int]),
    (
        "tfgnn_graph_gather_reduce",
        c_int,
        [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int,
         c_int, c_int, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_graph_gather_dot_supported", c_int, [c_int, c_int]),
    (
        "tfgnn_graph_gather_reduce_dot",
        c_int,
        [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_edge_pair_combine", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    ("tfgnn_graph_original_order", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_gemm_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64]),
    (
        "tfgnn_gemm_grad_epilogue",
        c_int,
        [c_int, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
         c_int, c_void_p, c_int64, c_int, c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_gemm_gathered",
        c_int,
        [c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
         c_int, c_int, c_void_p],
    ),
    ("tfgnn_gemm_set_mode", c_int, [c_int]),
    ("tfgnn_gemm_get_mode", c_int, []),
    (
        "tfgnn_gemm",
        c_int,
        [c_int, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
         c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_gemm_grouped_rows",
        c_int,
        [c_int, c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p,
         c_int64, c_int, c_void_p],
    ),
    (
        "tfgnn_gemm_grouped_rows_grad",
        c_int,
        [c_int, c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p,
         c_int64, c_int, c_void_p, c_int64, c_void_p],
    ),
    ("tfgnn_gemm_grouped_k_workspace_bytes", c_size_t, [c_int, c_int64, c_int64, c_int64]),
    (
        "tfgnn_gemm_grouped_k",
        c_int,
        [c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
         c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_graph_nonempty_offsets", c_int, [c_void_p, c_int, POINTER(c_int32)]),
    ("tfgnn_activation_forward", c_int, [c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tfgnn_activation_backward", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tfgnn_activation_backward_mul", c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    (
        "tfgnn_gemm_gru",
        c_int,
        [c_int64, c_int, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_gemm_gru2", c_int, [c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    ("tfgnn_gru_gates_forward", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    (
        "tfgnn_gru_gates_backward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p],
    ),
    ("tfgnn_gru_gates_backward_sp_workspace_bytes", c_size_t, [c_int64, c_int]),
    (
        "tfgnn_gru_gates_backward_sp",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
         c_int, c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_gru_gates_backward_sp_dropout",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, ctypes.c_uint64, c_void_p,
         c_int64, c_int, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_colsum_workspace_bytes", c_size_t, [c_int64, c_int]),
    ("tfgnn_colsum", c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("tfgnn_add_scale", c_int, [c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p]),
    ("tfgnn_rgat_node_scores", c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_rgat_edge_scores", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    ("tfgnn_rgat_edge_node_op", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    ("tfgnn_rgat_edge_dot", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    (
        "tfgnn_rgat_edge_softmax_backward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p],
    ),
    ("tfgnn_rgat_scores_backward", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    ("tfgnn_rgat_scores_backward_sp", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_rgat_attention_workspace_bytes", c_size_t, [c_void_p, c_int]),
    ("tfgnn_rgat_attention_forward", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("tfgnn_rgat_attention_backward", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("tfgnn_rgat_alpha_grad_workspace_bytes", c_size_t, [c_int64, c_int, c_int]),
    ("tfgnn_rgat_alpha_grad", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    (
        "tfgnn_layernorm_forward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
    (
        "tfgnn_layernorm_backward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_segment_offsets", c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    ("tfgnn_segment_offsets_async", c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_clip", c_int, [c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p]),
    ("tfgnn_clip_backward", c_int, [c_void_p, c_void_p, c_int64, c_float, c_float, c_void_p, c_void_p]),
    ("tfgnn_segment_softmax", c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    ("tfgnn_segment_weighted_sum", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    (
        "tfgnn_segment_weighted_sum_backward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_segment_softmax_backward", c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    ("tfgnn_dropout_forward", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, ctypes.c_uint64, c_void_p]),
    ("tfgnn_film_edge_forward", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    ("tfgnn_film_edge_backward", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                         c_void_p]),
    ("tfgnn_sp_gemm_nt_set_splitk_workspace", c_int, [c_void_p, ctypes.c_size_t]),
    ("tfgnn_sp_gemm_nt_splitk_status", c_int, [c_int, c_void_p, c_void_p]),
    ("tfgnn_dropout_epoch_advance", c_int, [c_void_p]),
    ("tfgnn_dropout_epoch_set", c_int, [ctypes.c_uint32, c_void_p]),
    ("tfgnn_dropout_epoch_get", c_int, [c_void_p, c_void_p]),
    ("tfgnn_dropout_forward_sp", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, ctypes.c_uint64, c_void_p, c_int64,
                                         c_void_p, c_void_p]),
    ("tfgnn_transpose_batched", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    (
        "tfgnn_edge_aggregate_backward",
        c_int,
        [c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p,
         c_void_p, c_int, c_void_p, c_void_p],
    ),
    (
        "tfgnn_film_combine_forward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p],
    ),
    (
        "tfgnn_film_combine_backward",
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_batch_offset_edges", c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_batch_node_to_graph_map", c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    ("tfgnn_adjacency_append", c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    ("tfgnn_adjacency_self_loops", c_int, [c_int64, c_void_p, c_void_p]),
    ("tfgnn_adjacency_in_degrees", c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    ("tfgnn_permute_021", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    ("tfgnn_mul", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tfgnn_task_metrics_workspace_bytes", c_size_t, []),
    (
        "tfgnn_sigmoid_ce_metrics",
        c_int,
        [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_regression_metrics", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    (
        "tfgnn_binary_ce_metrics",
        c_int,
        [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_softmax_ce_workspace_bytes", c_size_t, []),
    (
        "tfgnn_softmax_ce_metrics",
        c_int,
        [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
         c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_graph_gather_reduce_sp",
        c_int,
        [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_graph_gather_reduce_sp_keep_empty",
        c_int,
        [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p,
         c_void_p, c_size_t, c_int, c_void_p],
    ),
    ("tfgnn_sp_gemm_tn_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int]),
    ("tfgnn_sp_gemm_tn_grouped_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64, c_int, c_int]),
    (
        "tfgnn_sp_gemm_tn_grouped",
        c_int,
        [c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p,
         c_void_p, c_int64, c_int64, c_int64, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_sp_gemm_tn_wide_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64, c_int64, c_int]),
    (
        "tfgnn_sp_gemm_tn_wide",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p,
         c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_size_t, c_void_p],
    ),
    (
        "tfgnn_sp_gemm_tn",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p,
         c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_absmax", c_int, [c_void_p, c_int64, c_float, c_void_p, c_void_p]),
    ("tfgnn_sp_inv_scale_from_bound", c_int, [c_void_p, c_void_p, c_void_p]),
    ("tfgnn_sp_bytes", c_size_t, [c_int64, c_int64]),
    (
        "tfgnn_sp_split_rows",
        c_int,
        [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_sp_split_cols", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    (
        "tfgnn_sp_gemm_nt",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p],
    ),
    (
        "tfgnn_sp_gemm_nt_sp",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p],
    ),
    ("tfgnn_aux_launch", c_int, [c_void_p, c_int, c_void_p]),
    (
        "tfgnn_sp_split_rows_job",
        c_int,
        [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p],
    ),
    ("tfgnn_sp_split_cols_job", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    ("tfgnn_sp_split_cols_two_pass_bytes", c_size_t, [c_int64, c_int64]),
    ("tfgnn_sp_split_cols_jobs", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p,
                                         c_void_p]),
    (
        "tfgnn_graph_gather_reduce_sp_deferred",
        c_int,
        [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
         c_size_t, c_void_p, c_void_p],
    ),
    (
        "tfgnn_sp_gemm_nt_dropout",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float, c_void_p, c_int64, c_void_p, c_float,
         ctypes.c_uint64, c_void_p, c_void_p, c_void_p],
    ),
    (
        "tfgnn_sp_gemm_nt_grouped",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
         c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64,
         c_void_p, c_void_p],
    ),
    ("tfgnn_sp_gather_rows", c_int, [c_void_p, c_int64, c_void_p, c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64,
                                     c_void_p, c_void_p]),
    (
        "tfgnn_sp_gemm_nt_rows",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float, c_void_p, c_int64, c_void_p, c_float,
         ctypes.c_uint64, c_void_p, c_void_p, c_void_p],
    ),
]

# layer-level entry points (include/tfgnn.h, round 6): the argument structs travel by pointer
_SIGNATURES += [
    ("tfgnn_mp_forward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_mp_backward", c_int, [c_void_p, c_void_p]),
]

# the reduce pass of a weight-gradient product carried by the next NT launch (include/tfgnn.h tfgnn_tn_reduce_job)
_SIGNATURES += [
    (
        "tfgnn_sp_gemm_tn_product",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p,
         c_void_p, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_size_t, c_void_p, c_void_p],
    ),
    ("tfgnn_tn_reduce_launch", c_int, [c_void_p, c_void_p]),
    ("tfgnn_tn_reduce_counts", c_int, [POINTER(c_int64), c_int]),
    (
        "tfgnn_sp_gemm_nt_rows_tail",
        c_int,
        [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
         c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_float, c_void_p, c_int64, c_void_p, c_float,
         ctypes.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p],
    ),
]

# graph readout (include/tfgnn.h "Graph readout", csrc/pool_fused.hip)
_SIGNATURES += [
    ("tfgnn_pool_workspace_bytes", c_size_t, [c_int64, c_int64, c_int, c_int, c_int]),
    ("tfgnn_pool_forward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_pool_backward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_pool_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
POOL_SOFTMAX, POOL_SIGMOID, POOL_NONE, POOL_AVERAGE = range(4)  # tfgnn_pool_kind
POOL_CHUNK_NODES = 128  # TFGNN_POOL_CHUNK_NODES

# optimizer step (include/tfgnn.h "Optimizer step", csrc/optim.hip): descriptors and config travel by pointer
_SIGNATURES += [
    ("tfgnn_optimizer_workspace_bytes", c_size_t, [c_void_p, c_int, c_int]),
    ("tfgnn_optimizer_apply", c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    ("tfgnn_optimizer_iterations_get", c_int, [c_void_p, c_void_p, c_void_p]),
    ("tfgnn_optimizer_iterations_set", c_int, [c_void_p, c_int64, c_void_p]),
    ("tfgnn_optimizer_launch_count", c_int64, []),
    # the row-sparse step: dense tensors, row tensors (OptRowTensor array), config
    ("tfgnn_optimizer_rows_workspace_bytes", c_size_t, [c_void_p, c_int, c_void_p, c_int, c_int]),
    ("tfgnn_optimizer_apply_rows", c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
]
OPT_MAX_ROW_TENSORS = 8  # include/tfgnn.h TFGNN_OPT_MAX_ROW_TENSORS

# batch assembly from a device-resident fold (include/tfgnn.h, csrc/batch.hip): the argument struct travels by pointer
_SIGNATURES += [
    ("tfgnn_batch_assemble", c_int, [c_void_p, c_void_p]),
    ("tfgnn_batch_assemble_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
BATCH_MAX_EDGE_TYPES = 48  # TFGNN_BATCH_MAX_EDGE_TYPES
BATCH_MAX_COLUMNS = 8  # TFGNN_BATCH_MAX_COLUMNS
BATCH_MAX_NODE_COLUMNS = 4  # TFGNN_BATCH_MAX_NODE_COLUMNS

# link prediction with a DistMult decoder (include/tfgnn.h, csrc/link.hip)
_SIGNATURES += [
    ("tfgnn_distmult_ce_workspace_bytes", c_size_t, []),
    (
        "tfgnn_distmult_ce_metrics",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_distmult_backward_workspace_bytes", c_size_t, [c_int64, c_int64]),
    (
        "tfgnn_distmult_backward",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
         c_void_p, c_int64, c_int, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_distmult_rank_workspace_bytes", c_size_t, [c_int64]),
    (
        "tfgnn_distmult_rank",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_link_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
# ... and with a ComplEx decoder: the same argument lists; the rank workspace size also takes D
_SIGNATURES += [
    ("tfgnn_complex_ce_workspace_bytes", c_size_t, []),
    (
        "tfgnn_complex_ce_metrics",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p,
         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_complex_backward_workspace_bytes", c_size_t, [c_int64, c_int64]),
    (
        "tfgnn_complex_backward",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64,
         c_void_p, c_int64, c_int, c_void_p, c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_complex_rank_workspace_bytes", c_size_t, [c_int64, c_int64]),
    (
        "tfgnn_complex_rank",
        c_int,
        [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
         c_void_p, c_size_t, c_void_p],
    ),
    ("tfgnn_complex_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
LINK_CHUNK = 256  # csrc/link.hip LINK_CHUNK: list positions per chunk of the backward passes

# neighbour sampling and the row gather of a sampled batch (include/tfgnn.h "Neighbour sampling", csrc/sample.hip)
_SIGNATURES += [
    ("tfgnn_neighbor_sample_workspace_bytes", c_size_t, [c_int64, c_int, c_int64]),
    ("tfgnn_neighbor_sample", c_int, [c_void_p, c_void_p]),
    ("tfgnn_gather_node_rows", c_int, [c_void_p, c_void_p]),
    ("tfgnn_sample_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
# R-GCN basis decomposition (include/tfgnn.h "R-GCN basis decomposition", csrc/basis.hip)
_SIGNATURES += [
    ("tfgnn_basis_workspace_bytes", c_size_t, [c_int64, c_int64, c_int, c_int, c_int, c_int64, c_int64]),
    ("tfgnn_basis_gather_forward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_basis_gather_backward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_basis_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
BASIS_MAX_BASES = 64  # csrc/basis.hip: 1 <= num_bases <= 64
# R-GCN block-diagonal decomposition (include/tfgnn.h "R-GCN block-diagonal decomposition", csrc/blockdiag.hip)
_SIGNATURES += [
    ("tfgnn_blockdiag_workspace_bytes", c_size_t, [c_int, c_int, c_int, c_int64, c_int64, c_int64]),
    ("tfgnn_blockdiag_forward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_blockdiag_backward", c_int, [c_void_p, c_void_p]),
    ("tfgnn_blockdiag_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
# edge dropout of the layers that read the graph through graph_scales' arrays (include/tfgnn.h, csrc/edge_dropout.hip)
_SIGNATURES += [
    ("tfgnn_graph_scales_edge_dropout", c_int,
     [c_void_p, c_int, c_int, c_void_p, ctypes.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tfgnn_edge_dropout_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
# negatives and triple tables of a link-prediction batch on the device (include/tfgnn.h, csrc/negatives.hip)
_SIGNATURES += [
    ("tfgnn_triples_draw_negatives", c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, ctypes.c_uint64, c_int, c_void_p]),
    ("tfgnn_triple_tables_workspace_bytes", c_size_t, [c_int64, c_int64, c_int64]),
    ("tfgnn_triple_tables_build", c_int,
     [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("tfgnn_negatives_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
# node embeddings: the dense table gradient of a row lookup with distinct ids (include/tfgnn.h, csrc/embedding.hip)
_SIGNATURES += [
    ("tfgnn_embedding_scatter_rows", c_int,
     [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    ("tfgnn_embedding_launch_count", c_int64, []),
]
# one mini-batch of link-prediction triples: gather, negatives, seeds, local ids (include/tfgnn.h "Triple batches",
# csrc/triple_batch.hip)
_SIGNATURES += [
    ("tfgnn_triple_batch_workspace_bytes", c_size_t, [c_int64]),
    ("tfgnn_triple_batch_build", c_int, [c_void_p, c_void_p]),
    ("tfgnn_triple_batch_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
TRIPLE_BATCH_SEED_OVERFLOW, TRIPLE_BATCH_BAD_POSITIVE_ID, TRIPLE_BATCH_BAD_ENDPOINT = 1, 2, 4  # TFGNN_TRIPLE_BATCH_*
TRIPLE_BATCH_LAUNCHES = 6  # per tfgnn_triple_batch_build call
# a batch's positives out of its sampled subgraph (include/tfgnn.h "Excluding a batch's positives", csrc/sample_exclude.hip)
_SIGNATURES += [
    ("tfgnn_sample_exclude_workspace_bytes", c_size_t, [c_int, c_void_p]),
    ("tfgnn_sample_exclude_edges", c_int, [c_void_p, c_void_p]),
    ("tfgnn_sample_exclude_launch_counts", c_int, [POINTER(c_int64), c_int]),
]
SAMPLE_EXCLUDE_LAUNCHES = 4  # TFGNN_SAMPLE_EXCLUDE_LAUNCHES, per tfgnn_sample_exclude_edges call
SAMPLE_EXCLUDE_BAD_RELATION, SAMPLE_EXCLUDE_BAD_ENDPOINT = 32, 64  # TFGNN_SAMPLE_EXCLUDE_*
TRIPLE_SORT_TILE = 8192  # csrc/negatives.hip TS_TILE: keys per workgroup of the table sort
TRIPLE_SORT_DIGIT_BITS = 9  # csrc/negatives.hip TS_DIGIT_BITS
BLOCKDIAG_MAX_BLOCK = 64  # csrc/blockdiag.hip MAX_BLOCK: D / num_blocks and H / num_blocks at most
BLOCKDIAG_CHUNK = 256  # csrc/blockdiag.hip DQ_CHUNK: list positions per chunk of dQb's first stage
SAMPLE_MAX_HOPS = 8  # TFGNN_SAMPLE_MAX_HOPS
SAMPLE_META_STATUS, SAMPLE_META_NODES, SAMPLE_META_EDGES = 0, 1, 2  # TFGNN_SAMPLE_META_*
SAMPLE_NODE_OVERFLOW, SAMPLE_EDGE_OVERFLOW, SAMPLE_REPEATED_SEED, SAMPLE_BAD_SEED, SAMPLE_BAD_STORE = 1, 2, 4, 8, 16


def sample_meta_words(num_edge_types: int, num_hops: int) -> int:
    """TFGNN_SAMPLE_META_WORDS: status, node count, the edge counts, hop_ptr [K + 2]"""
    return 2 + num_edge_types + num_hops + 2


EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]
ABI_VERSION = 5  # include/tfgnn.h TFGNN_ABI_VERSION


class AuxJob(ctypes.Structure):
    """tfgnn_aux_job (include/tfgnn.h): one small pass of a merged launch"""

    _fields_ = [("kind", c_int), ("num_blocks", ctypes.c_uint), ("payload", ctypes.c_ubyte * 248)]


class TnReduceJob(ctypes.Structure):
    """tfgnn_tn_reduce_job (include/tfgnn.h): the reduce pass a deferred weight-gradient product hands back"""

    _fields_ = [("num_blocks", ctypes.c_uint), ("reserved", ctypes.c_uint), ("payload", ctypes.c_ubyte * 184)]


class MpForwardArgs(ctypes.Structure):
    """tfgnn_mp_forward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("kind", c_int), ("graph", c_void_p), ("view", c_int), ("x", c_void_p), ("ldx", c_int64),
        ("in_dim", c_int), ("hidden_dim", c_int), ("row_scale", c_void_p), ("w", c_void_p), ("wt_sp", c_void_p),
        ("ld_wt_sp_bytes", c_int64), ("wt_inv_scale", c_void_p), ("agg_sp", c_void_p), ("agg_inv_scale", c_void_p), ("bias", c_void_p),
        ("act", c_int), ("dropout_rate", ctypes.c_float), ("dropout_seed", ctypes.c_uint64), ("tile_kmask", c_void_p),
        ("row_map", c_void_p), ("out", c_void_p), ("ld_out", c_int64), ("out_sp", c_void_p), ("ld_out_sp_bytes", c_int64),
        ("out_inv_scale", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t), ("agg_filled", c_int),
    ]


class MpBackwardArgs(ctypes.Structure):
    """tfgnn_mp_backward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("kind", c_int), ("graph", c_void_p), ("d_pre", c_void_p), ("ld_d_pre", c_int64),
        ("in_dim", c_int), ("hidden_dim", c_int), ("edge_weight", c_void_p), ("w", c_void_p), ("wh_sp", c_void_p),
        ("ld_wh_sp_bytes", c_int64), ("wh_inv_scale", c_void_p), ("g_sp", c_void_p), ("g_inv_scale", c_void_p), ("dx", c_void_p),
        ("ld_dx", c_int64), ("accumulate", c_int), ("mul", c_void_p), ("ld_mul", c_int64), ("act_of_saved", c_int), ("saved", c_void_p),
        ("ld_saved", c_int64), ("saved_scale", ctypes.c_float), ("dropout_rate", ctypes.c_float), ("dropout_seed", ctypes.c_uint64),
        ("dx_sp", c_void_p), ("ld_dx_sp_bytes", c_int64), ("dx_inv_scale", c_void_p), ("tile_kmask", c_void_p), ("a_rows", c_void_p),
        ("row_map", c_void_p), ("dw", c_void_p), ("x_sp", c_void_p), ("ld_x_sp_bytes", c_int64), ("x_inv_scale", c_void_p),
        ("tn_workspace", c_void_p), ("tn_workspace_bytes", ctypes.c_size_t), ("workspace", c_void_p),
        ("workspace_bytes", ctypes.c_size_t), ("g_filled", c_int),
    ]


class PoolForwardArgs(ctypes.Structure):
    """tfgnn_pool_forward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("kind", c_int), ("V", c_int64), ("G", c_int64), ("GD", c_int), ("heads", c_int),
        ("ptr", c_void_p), ("T", c_void_p), ("ldT", c_int64), ("S", c_void_p), ("ldS", c_int64), ("lo", c_float), ("hi", c_float),
        ("out", c_void_p), ("w", c_void_p), ("ldw", c_int64), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class PoolBackwardArgs(ctypes.Structure):
    """tfgnn_pool_backward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("kind", c_int), ("V", c_int64), ("G", c_int64), ("GD", c_int), ("heads", c_int),
        ("ptr", c_void_p), ("ids", c_void_p), ("dOut", c_void_p), ("T", c_void_p), ("ldT", c_int64), ("w", c_void_p),
        ("ldw", c_int64), ("lo", c_float), ("hi", c_float), ("dT", c_void_p), ("lddT", c_int64), ("dS", c_void_p),
        ("lddS", c_int64), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class BasisForwardArgs(ctypes.Structure):
    """tfgnn_basis_forward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("graph", c_void_p), ("B", c_int), ("D", c_int), ("coeff", c_void_p), ("X", c_void_p),
        ("ldX", c_int64), ("edge_weight_by_dst", c_void_p), ("node_scale", c_void_p), ("Z", c_void_p), ("ldZ", c_int64),
        ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class BasisBackwardArgs(ctypes.Structure):
    """tfgnn_basis_backward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("graph", c_void_p), ("B", c_int), ("D", c_int), ("coeff", c_void_p), ("dZ", c_void_p),
        ("lddZ", c_int64), ("X", c_void_p), ("ldX", c_int64), ("edge_weight_by_dst", c_void_p), ("edge_weight_by_src", c_void_p),
        ("node_scale", c_void_p), ("dX", c_void_p), ("lddX", c_int64), ("dcoeff", c_void_p), ("workspace", c_void_p),
        ("workspace_bytes", ctypes.c_size_t),
    ]


class BlockdiagForwardArgs(ctypes.Structure):
    """tfgnn_blockdiag_forward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("graph", c_void_p), ("C", c_int), ("D", c_int), ("H", c_int), ("Qb", c_void_p),
        ("X", c_void_p), ("ldX", c_int64), ("edge_weight_by_dst", c_void_p), ("node_scale", c_void_p), ("pre", c_void_p),
        ("ldpre", c_int64), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class BlockdiagBackwardArgs(ctypes.Structure):
    """tfgnn_blockdiag_backward_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("graph", c_void_p), ("C", c_int), ("D", c_int), ("H", c_int), ("Qb", c_void_p),
        ("dPre", c_void_p), ("lddPre", c_int64), ("X", c_void_p), ("ldX", c_int64), ("edge_weight_by_dst", c_void_p),
        ("edge_weight_by_src", c_void_p), ("node_scale", c_void_p), ("dX", c_void_p), ("lddX", c_int64), ("dQb", c_void_p),
        ("list_to_dst", c_void_p), ("chunk_first", c_void_p), ("chunk_count", c_void_p), ("type_chunk_ptr", c_void_p),
        ("num_chunks", c_int64), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class BatchAssembleArgs(ctypes.Structure):
    """tfgnn_batch_assemble_args (include/tfgnn.h), field for field.  The pointer tables are host arrays (c_void_p * n,
    c_int64 * n) that the caller keeps alive for the duration of the call."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("num_edge_types", c_int), ("num_columns", c_int), ("num_graphs", c_int64),
        ("store_nodes", c_int64), ("feature_dim", c_int64), ("node_ptr", c_void_p), ("features", c_void_p), ("edge_ptr", c_void_p),
        ("edges", c_void_p), ("columns", c_void_p), ("order_len", c_int64), ("order", c_void_p), ("pos_node_ptr", c_void_p),
        ("pos_edge_ptr", c_void_p), ("p0", c_int64), ("p1", c_int64), ("num_nodes", c_int64), ("num_edges", c_void_p),
        ("node_features", c_void_p), ("node_to_graph_map", c_void_p), ("adjacency_lists", c_void_p), ("column_out", c_void_p),
        ("bad_flag", c_void_p), ("num_node_columns", c_int), ("node_column_widths", c_void_p), ("node_columns", c_void_p),
        ("node_column_out", c_void_p),
    ]


class NeighborSampleArgs(ctypes.Structure):
    """tfgnn_neighbor_sample_args (include/tfgnn.h), field for field.  The pointer tables and ``fanouts`` are host arrays
    that the caller keeps alive for the duration of the call."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("num_edge_types", c_int), ("num_hops", c_int), ("num_nodes", c_int64),
        ("in_ptr", c_void_p), ("in_src", c_void_p), ("store_edges", c_void_p), ("fanouts", c_void_p), ("seed", ctypes.c_uint64),
        ("num_seeds", c_int64), ("seeds", c_void_p), ("node_capacity", c_int64), ("edge_capacity", c_void_p), ("nodes", c_void_p),
        ("adjacency_lists", c_void_p), ("meta", c_void_p), ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class GatherNodeRowsArgs(ctypes.Structure):
    """tfgnn_gather_node_rows_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("store_nodes", c_int64), ("num_rows", c_int64), ("num_seeds", c_int64), ("nodes", c_void_p),
        ("feature_dim", c_int64), ("features", c_void_p), ("node_features", c_void_p), ("num_node_columns", c_int),
        ("node_column_widths", c_void_p), ("node_columns", c_void_p), ("node_column_out", c_void_p), ("seed_only", c_void_p),
        ("bad_flag", c_void_p),
    ]


class TripleBatchArgs(ctypes.Structure):
    """tfgnn_triple_batch_args (include/tfgnn.h), field for field"""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("num_nodes", c_int64), ("num_positives", c_int64), ("positives", c_void_p),
        ("batch_size", c_int64), ("positive_ids", c_void_p), ("negatives_per_positive", c_int64), ("seed", ctypes.c_uint64),
        ("seed_capacity", c_int64), ("triples", c_void_p), ("local_triples", c_void_p), ("seeds", c_void_p), ("meta", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class SampleExcludeArgs(ctypes.Structure):
    """tfgnn_sample_exclude_args (include/tfgnn.h), field for field.  The two type tables, the capacities and the pointer
    table are host arrays that the caller keeps alive for the duration of the call."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("num_edge_types", c_int), ("num_relations", c_int), ("num_seeds", c_int64),
        ("num_positives", c_int64), ("positives", c_void_p), ("fwd_type", c_void_p), ("inv_type", c_void_p),
        ("edge_capacity", c_void_p), ("adjacency_lists", c_void_p), ("meta", c_void_p), ("record", c_void_p),
        ("workspace", c_void_p), ("workspace_bytes", ctypes.c_size_t),
    ]


class OptConfig(ctypes.Structure):
    """tfgnn_opt_config (include/tfgnn.h), field for field.  The tensors go in as an int64 array [n, 8] laid out like
    tfgnn_opt_tensor (value, ld_value, grad, ld_grad, rows, cols, slot0, slot1)."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t), ("kind", c_int), ("clip", c_int), ("clip_value", c_float), ("momentum", c_float),
        ("rho", c_float), ("beta_1", c_float), ("beta_2", c_float), ("epsilon", c_float), ("schedule", c_int),
        ("learning_rate", c_float), ("initial_learning_rate", c_float), ("final_learning_rate", c_float), ("power", c_float),
        ("warmup_steps", c_int64), ("decay_steps", c_int64), ("state", c_void_p), ("workspace", c_void_p),
        ("workspace_bytes", ctypes.c_size_t),
    ]


class OptRowTensor(ctypes.Structure):
    """tfgnn_opt_row_tensor (include/tfgnn.h), field for field: a table and the row gradient (grad_rows, ids) against it."""

    _fields_ = [
        ("value", c_void_p), ("ld_value", c_int64), ("grad_rows", c_void_p), ("ld_grad", c_int64), ("ids", c_void_p),
        ("n", c_int64), ("N", c_int64), ("cols", c_int64), ("slot0", c_void_p), ("slot1", c_void_p), ("bad_flag", c_void_p),
    ]


_lib = None


class TfgnnError(RuntimeError):
    pass


def load():
    """Load libtfgnn.so (once).  Raises RuntimeError when it is missing - never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built. Run `python -m tf2_gnn_amd.build` "
            "(hipcc --offload-arch=gfx950). tf2_gnn_amd has no CPU fallback."
        )
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover
        raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, restype, argtypes in _SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.tfgnn_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} speaks ABI version {lib.tfgnn_abi_version()}, this binding was written against {ABI_VERSION} "
                           "(include/tfgnn.h TFGNN_ABI_VERSION): rebuild with `python -m tf2_gnn_amd.build`")
    _lib = lib
    return lib


def check(status: int):
    if status == 0:
        return
    msg = load().tfgnn_last_error().decode("utf-8", "replace")
    if status in (-1, -2):
        # same convention as the reference's Python layer: bad arguments / indices -> ValueError
        raise ValueError(f"tfgnn: {msg}")
    raise TfgnnError(f"tfgnn (status {status}): {msg}")
