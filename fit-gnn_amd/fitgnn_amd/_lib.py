"""ctypes binding of libfitgnn_hip.so (the C ABI declared in include/fitgnn_hip.h).

The product has NO CPU fallback: if the shared library is missing or a call fails, an exception
is raised.  Build it with `python __graft_entry__.py` or `make -C fit-gnn_amd/csrc`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libfitgnn_hip.so")

c_i32, c_i64, c_u32, c_u64, c_f32, c_size = (ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64,
                                              ctypes.c_float, ctypes.c_size_t)
ptr = ctypes.c_void_p

EPI_BIAS, EPI_ELU, EPI_DROPOUT, EPI_SEED_DEVICE = 1, 2, 4, 8
SPMM_GATHER = 0x100
MAX_K = 16
MATCH_HEAVY_EDGE, MATCH_ALGEBRAIC_JC = 0, 1
MATCH_SMALL_MAX_NODES, MATCH_SMALL_MAX_NNZ, MATCH_SMALL_MAX_K, MATCH_SMALL_LDS_BUDGET = 128, 1024, 12, 65536
MATCH_DONE, MATCH_TOO_BIG, MATCH_BAD_INPUT = 1, 2, 3
QUALITY_MAX_K = 64

# name -> (restype, argtypes); mirrors include/fitgnn_hip.h one to one
SIGNATURES = {
    "fitgnn_abi_version": (ctypes.c_int, []),
    "fitgnn_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "fitgnn_stream_copy_f32": (ctypes.c_int, [ptr, ptr, c_i64, ptr]),
    "fitgnn_spmm_default_window_rows": (ctypes.c_int, []),
    "fitgnn_spmm_max_window_rows": (ctypes.c_int, [c_i32]),
    "fitgnn_gcn_norm_csr_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, ptr]),
    "fitgnn_spmm_csr_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr, ptr,
                                           ptr, c_i32, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr]),
    "fitgnn_spmm_csr_blocks_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr,
                                                  ptr, ptr, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr]),
    "fitgnn_spmm_csr_dz_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr, ptr,
                                              ptr, c_i32, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr, ptr]),
    "fitgnn_spmm_csr_blocks_dz_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr,
                                                     ptr, ptr, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr, ptr]),
    "fitgnn_lanczos_parts": (c_i32, [c_i32]),
    "fitgnn_lanczos_spmv_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, ctypes.c_double, ctypes.c_double, ptr]),
    "fitgnn_lanczos_project_f64": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i32, ptr, ptr, ptr]),
    "fitgnn_lanczos_reduce_f64": (ctypes.c_int, [ptr, c_i32, c_i32, ptr, ptr]),
    "fitgnn_lanczos_finish_f64": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i32, ptr, ptr, ptr, ptr, c_i32, ptr]),
    "fitgnn_lanczos_rotate_f64": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i32, ptr, c_i64, c_i32, ptr]),
    "fitgnn_spmm_csr_stream_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr, c_i32, ptr, ptr,
                                                  ptr, c_u32, c_f32, c_u64, ptr, ptr]),
    "fitgnn_spmm_csr_stream_dz_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr, c_i32, ptr, ptr,
                                                     ptr, c_u32, c_f32, c_u64, ptr, ptr, ptr]),
    "fitgnn_spmm_rows_compact_parts": (c_i32, [c_i32]),
    "fitgnn_spmm_rows_compact_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, ptr, c_i64, c_i32, c_i32, ptr]),
    "fitgnn_spmm_rows_compact_dz_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, ptr, c_i64, c_i32, c_i32, ptr, c_u32, c_f32,
                                                       c_u64, ptr, ptr, ptr]),
    "fitgnn_two_hop_rows_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, c_i32, ptr, c_i32, ptr, c_i32, c_u32, c_f32, c_u64, ptr, ptr, c_i64, ptr]),
    "fitgnn_spmm_two_hop_blocks_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i32, ptr, ptr, ptr, ptr, ptr, c_i64,
                                                      c_i32, ptr, ptr, c_u32, c_f32, c_u64, ptr, ptr, ptr]),
    "fitgnn_segment_sum_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, c_i64, c_i32, ptr, c_i64, ptr]),
    "fitgnn_segment_max_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, c_i64, c_i32, ptr, ptr, ptr]),
    "fitgnn_segment_max_bwd_f32": (ctypes.c_int, [ptr, ptr, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_segment_expand_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, c_i32, ptr, ptr]),
    "fitgnn_make_tiles_host": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i64, ptr]),
    "fitgnn_split_blocks_host": (ctypes.c_int, [ptr, c_i64, ptr, c_i32, c_i64, c_i32, ptr, c_i64, ptr, ptr, ptr, ptr, c_i64, ptr]),
    "fitgnn_plan_tiles_host": (ctypes.c_int, [ptr, ptr, c_i32, c_i32, ptr, c_i32, c_i32, c_i32, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_epilogue_bwd_workspace_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_epilogue_bwd_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i32, c_i32, c_u32, c_f32, c_u64, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_head_max_classes": (ctypes.c_int, []),
    "fitgnn_head_max_classes_wide": (ctypes.c_int, []),
    "fitgnn_epilogue_bwd_head_supported": (ctypes.c_int, [c_i32, c_i32, c_i32]),
    "fitgnn_epilogue_bwd_head_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_epilogue_bwd_head_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr, c_i32, c_i32, c_u32, c_f32, c_u64, ptr, ptr, ptr,
                                                   ptr, c_size, ptr]),
    "fitgnn_epilogue_bwd_head_rows_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr, c_i32, c_i32, ptr, c_i32, c_u32, c_f32, c_u64, ptr,
                                                        ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_epilogue_bwd_rows_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i32, c_i32, ptr, c_i32, c_u32, c_f32, c_u64, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_spmm_epilogue_bwd_supported": (ctypes.c_int, [c_i32, c_i32, c_i32]),
    "fitgnn_spmm_epilogue_bwd_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_spmm_epilogue_bwd_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, c_i32, ptr, ptr, ptr, c_i32, ptr, ptr, c_i32, c_i32,
                                                   c_u32, c_f32, c_u64, ptr, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_gat_scores_f32": (ctypes.c_int, [ptr, c_i64, c_i32, c_i32, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_gat_edge_softmax_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_f32, c_i32, ptr, ptr]),
    "fitgnn_sddmm_csr_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, ptr]),
    "fitgnn_sddmm_csr_rows_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, ptr, c_i32, c_i32, ptr, ptr]),
    "fitgnn_gat_softmax_bwd_rows_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_f32, ptr, c_i32, ptr, ptr, ptr]),
    "fitgnn_gat_softmax_bwd_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_f32, c_i32, ptr, ptr, ptr]),
    "fitgnn_gat_heads_scores_f32": (ctypes.c_int, [ptr, c_i64, c_i32, c_i32, c_i32, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_gat_heads_edge_softmax_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_f32, c_i32, c_i64, c_i32, ptr, ptr]),
    "fitgnn_gat_heads_aggregate_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i64, c_i32, c_i32, ptr, ptr]),
    "fitgnn_gat_heads_sddmm_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, c_i64, c_i32, c_i64, c_i32, c_i32, ptr, ptr]),
    "fitgnn_gat_heads_softmax_bwd_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_f32, c_i32, c_i64, c_i32, ptr, ptr, ptr]),
    "fitgnn_l1_loss_f32": (ctypes.c_int, [ptr, ptr, c_i32, c_f32, ptr, ptr, ptr]),
    "fitgnn_softmax_nll_workspace_bytes": (c_size, [c_i32]),
    "fitgnn_softmax_nll_f32": (ctypes.c_int, [ptr, c_i64, c_i32, c_i32, ptr, ptr, c_i32, c_f32, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_adam_step_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, ptr, ptr]),
    "fitgnn_sum_leading_f32": (ctypes.c_int, [ptr, c_i32, c_i64, ptr, ptr]),
    "fitgnn_gemm_atb_workspace_bytes": (c_size, [c_i64, c_i32, c_i32]),
    "fitgnn_gemm_atb_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i64, c_i32, c_i32, ptr, ptr, ptr]),
    "fitgnn_gemm_nt_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i64, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_gemm_exact_workspace_bytes": (c_size, [c_i64, c_i32, c_i64, c_i32, c_i32]),
    "fitgnn_gemm_exact_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i64, c_i32, c_i64, c_i32, c_i64, ptr, c_i64, ptr, ptr]),
    "fitgnn_gemm_exact_plan": (ctypes.c_int, [c_i64, c_i32, c_i64, c_i32, c_i32, ptr, ptr, ptr]),
    "fitgnn_gemm_exact_epi_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i64, c_i32, c_i64, ptr, c_i64, ptr, ptr, c_u32, c_f32, c_u64, ptr, ptr,
                                                 ptr]),
    "fitgnn_gemm_exact_rows_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, ptr, c_i64, c_i32, ptr, c_i64, c_i32, c_i64, ptr, c_i64, ptr, ptr]),
    "fitgnn_gemm_exact_epi_rows_f32": (ctypes.c_int, [ptr, c_i64, ptr, ptr, c_i64, c_i64, c_i32, c_i64, ptr, c_i64, ptr, ptr, c_u32, c_f32,
                                                      c_u64, ptr, ptr, ptr]),
    "fitgnn_gemm_nt_presplit_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_gemm_nt_presplit_f32": (ctypes.c_int, [ptr, c_i64, c_i64, c_i32, c_i32, c_i32, ptr, ptr]),
    "fitgnn_gemm_nt_pre_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_gemm_nt_epilogue_bwd_workspace_bytes": (c_size, [c_i64, c_i32]),
    "fitgnn_gemm_nt_epilogue_bwd_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i64, c_i32, c_i32, ptr, ptr, ctypes.c_uint32, c_f32,
                                                       ctypes.c_uint64, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_colsum_partials_f32": (ctypes.c_int, [ptr, c_i32, c_i32, ptr, ptr]),
    "fitgnn_head_rows_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_head_rows_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i32, ptr, ptr, c_i32, c_i32, ptr, c_i64, c_i32, ptr]),
    "fitgnn_epilogue_fwd_rows_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i32, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr]),
    "fitgnn_dense_narrow_k_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_dense_narrow_k_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i64, c_i32, c_i32, c_i32, ptr, c_u32, c_f32, c_u64, ptr, ptr, c_i64, ptr]),
    "fitgnn_narrow_atb_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_narrow_atb_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_u32, c_f32, c_u64, ptr, ptr, c_i64, c_i32, c_i32, c_i32, ptr, ptr, ptr, c_size,
                                             ptr]),
    "fitgnn_adam_step_acc_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, ptr, ptr, c_i32, c_u64, ptr]),
    "fitgnn_pool_head_supported": (ctypes.c_int, [c_i32, c_i32]),
    "fitgnn_pool_head_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, c_i64, c_i32, ptr, ptr, ptr, c_i32, ptr, ptr, ptr]),
    "fitgnn_pool_head_bwd_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr, ptr, c_i64, c_i32, c_i32, ptr, ptr, ptr, ptr]),
    "fitgnn_colsum_narrow_workspace_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_colsum_narrow_f32": (ctypes.c_int, [ptr, c_i64, c_i32, c_i32, ptr, ptr, c_size, ptr]),
    "fitgnn_spmm_narrow_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_f32, ptr, c_f32, ptr, c_f32, ptr]),
    "fitgnn_spmm_narrow_padded_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_f32, ptr, c_f32, ptr, c_f32, ptr]),
    "fitgnn_appnp_unit_rows": (ctypes.c_int, [c_i32]),
    "fitgnn_appnp_unit_entries": (ctypes.c_int, []),
    "fitgnn_appnp_block_rows": (ctypes.c_int, []),
    "fitgnn_appnp_block_entries": (ctypes.c_int, []),
    "fitgnn_appnp_blocks_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, ptr, ptr, ptr, c_i32, c_i32, c_f32, c_i32, ptr]),
    "fitgnn_appnp_lds_bytes": (ctypes.c_int64, [c_i32, c_i32, c_i32]),
    "fitgnn_appnp_lds_max_bytes": (ctypes.c_int, []),
    "fitgnn_appnp_lds_items_per_thread": (ctypes.c_int, []),
    "fitgnn_appnp_lds_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, ptr, c_i32, c_i32, c_f32, c_i32, c_i32, c_i32, ptr]),
    "fitgnn_gather_rows_padded_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i64, ptr, c_i32, ptr]),
    "fitgnn_appnp_units_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, ptr, c_i32, c_i32, c_f32, c_i32, ptr]),
    "fitgnn_gcn_query_gather_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_sage_query_gather_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_gat_query_gather_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, c_f32, ptr, ptr, c_f32, ptr, c_i32, c_i32, ptr,
                                                   c_i64, ptr]),
    "fitgnn_gcn_query_tail_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_gcn_query_tail_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, c_i64, c_i32, ptr]),
    "fitgnn_mhgat_query_gather_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, ptr, ptr, c_i32, ptr, c_f32, ptr, ptr, c_f32, ptr, c_i32, c_i32,
                                                     ptr, c_i64, ptr]),
    "fitgnn_mhgat_query_tail_lds_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_mhgat_query_tail_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, c_i32, ptr, c_i64, c_i32, ptr]),
    "fitgnn_gcn_graph_query_hops_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_gcn_graph_query_hops_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_gcn_graph_query_tail_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_gcn_graph_query_tail_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i32, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, c_i32, c_i32, ptr, c_i64,
                                                       ptr]),
    "fitgnn_gin_query_hops_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, c_i64,
                                                 ptr]),
    "fitgnn_gin_query_tail_lds_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_gin_query_tail_f32": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, c_i32, ptr, c_i64, c_i32,
                                                 ptr]),
    "fitgnn_gin_graph_query_hops_lds_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_gin_graph_query_hops_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32,
                                                       c_i32, ptr, c_i64, ptr]),
    "fitgnn_gin_graph_query_tail_lds_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_gin_graph_query_tail_f32": (ctypes.c_int, [ptr, c_i64, ptr, c_i32, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, c_i32, c_i32,
                                                       c_i32, ptr, c_i64, ptr]),
    "fitgnn_gat_graph_query_hops_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_gat_graph_query_hops_f32": (ctypes.c_int, [ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, c_f32, ptr, ptr, c_f32, ptr, ptr, ptr, c_i32,
                                                       c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_sage_graph_query_hops_lds_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_sage_graph_query_hops_f32": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr, ptr, c_i32, c_i32, c_i32, ptr, c_i64, ptr]),
    "fitgnn_csr_row_sum_f32": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr]),
    "fitgnn_induced_edges_count": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, c_i64, ptr, ptr]),
    "fitgnn_induced_edges_fill": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, ptr]),
    "fitgnn_batch_offsets": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_batch_gather": (ctypes.c_int, [c_i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, ptr, c_i32, c_i32,
                                           c_i32, c_i32, c_i32, c_i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_i32, ptr, ptr, ptr, ptr, ptr,
                                           c_i32, ptr]),
    "fitgnn_closed_neighbourhoods": (ctypes.c_int, [ptr, ptr, c_i32, ptr, ptr, ptr]),
    "fitgnn_variation_costs_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i64, ptr, ptr, ptr, c_i32, ptr, ptr]),
    "fitgnn_variation_costs_batch_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i64, ptr, ptr, ptr, ptr, c_i32, ptr, ptr]),
    "fitgnn_greedy_select_workspace_bytes": (c_size, [c_i32, c_i64]),
    "fitgnn_greedy_select": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i64, c_i32, ptr, ptr, ptr, c_i64, ptr, ptr,
                                            ptr, ptr, c_size, ptr]),
    "fitgnn_greedy_select_batch_workspace_bytes": (c_size, [c_i32, c_i64, c_i32]),
    "fitgnn_greedy_select_batch": (ctypes.c_int, [ptr, ptr, ptr, ptr, ptr, c_i32, c_i64, c_i32, ptr, ptr, ptr, c_i32, ptr, ptr,
                                                  c_i64, ptr, ptr, ptr, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_build_assignment_workspace_bytes": (c_size, [c_i32]),
    "fitgnn_build_assignment": (ctypes.c_int, [c_i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_compose_levels": (ctypes.c_int, [c_i32, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_lift_adjacency_workspace_bytes": (c_size, [c_i32, c_i64, c_i32]),
    "fitgnn_lift_adjacency": (ctypes.c_int, [c_i32, ptr, ptr, ptr, ptr, ptr, c_i32, ptr, ptr, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_edge_list": (ctypes.c_int, [ptr, ptr, ptr, c_i32, ptr, ptr, ptr, ptr, c_i64, ptr, ptr]),
    "fitgnn_heavy_edge_proximity_workspace_bytes": (c_size, [c_i32]),
    "fitgnn_heavy_edge_proximity": (ctypes.c_int, [ptr, ptr, ptr, c_i32, ptr, ptr, ptr, c_i64, ptr, ptr, c_size, ptr]),
    "fitgnn_jc_proximity": (ctypes.c_int, [ptr, ptr, c_i64, ptr, c_i32, c_i64, ptr, ptr]),
    "fitgnn_affinity_proximity_workspace_bytes": (c_size, [c_i32, c_i64]),
    "fitgnn_affinity_proximity": (ctypes.c_int, [c_i32, ptr, ptr, c_i64, ptr, c_i32, c_i64, ptr, ptr, c_size, ptr]),
    "fitgnn_edge_variation_costs_f64": (ctypes.c_int, [ptr, ptr, c_i64, ptr, ptr, c_i32, c_i64, ptr, ptr]),
    "fitgnn_jacobi_vectors_workspace_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_jacobi_vectors_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, ptr, c_i32, c_i32, ptr, ptr, c_size, ptr]),
    "fitgnn_gauss_seidel_vectors_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, c_i32, ptr, ptr, c_i32, ptr, ptr]),
    "fitgnn_greedy_matching_workspace_bytes": (c_size, [c_i32, c_i64, c_i32]),
    "fitgnn_greedy_matching": (ctypes.c_int, [ptr, ptr, ptr, c_i32, ptr, ptr, ptr, c_i64, ptr, c_i32, ptr, ptr, c_i64, ptr, ptr, ptr,
                                              ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_match_small_lds_bytes": (c_size, [c_i32, c_i32, c_i32, c_i32]),
    "fitgnn_match_small": (ctypes.c_int, [c_i32, ptr, ptr, ptr, ptr, c_i32, c_i32, ctypes.c_double, c_i32, c_i32, ctypes.c_double, ptr,
                                          c_i64, ptr, c_i32, c_i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_pool_rows_workspace_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_pool_rows_f32": (ctypes.c_int, [ptr, ptr, c_i32, c_i32, ptr, c_i64, c_i32, ptr, c_i64, ptr, ptr, c_size, ptr]),
    "fitgnn_coarse_laplacian_workspace_bytes": (c_size, [c_i32, c_i64, c_i32]),
    "fitgnn_coarse_laplacian": (ctypes.c_int, [c_i32, ptr, ptr, ptr, c_i64, ptr, ptr, ptr, c_i32, ptr, ptr, ptr, ptr, ptr, c_size, ptr]),
    "fitgnn_project_lift_workspace_bytes": (c_size, [c_i32, c_i32]),
    "fitgnn_project_lift_f64": (ctypes.c_int, [ptr, ptr, c_i32, c_i32, ptr, c_i64, c_i32, ptr, c_i64, ptr, c_i64, ptr, c_size, ptr]),
    "fitgnn_laplacian_gram_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_laplacian_gram_f64": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i32, ptr, c_i64, c_i32, ptr, c_i64, c_i32, ptr, c_i64, ptr, c_size,
                                                 ptr]),
    "fitgnn_cross_atb_workspace_bytes": (c_size, [c_i32, c_i32, c_i32]),
    "fitgnn_cross_atb_f64": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, c_i64, c_i32, c_i32, ptr, c_i64, ptr, c_size, ptr]),
    "fitgnn_louvain_sweep_workspace_bytes": (c_size, [c_i64, c_i32]),
    "fitgnn_louvain_bucket_rows": (ctypes.c_int, [ptr, c_i64, c_i32, ptr, ptr, c_size, ptr]),
    "fitgnn_louvain_sweep": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, c_i64, ptr, ptr, ptr, c_i32, ptr, c_i32, ptr, ptr, c_size, ptr]),
    "fitgnn_louvain_stats": (ctypes.c_int, [ptr, ptr, ptr, ptr, c_i64, c_i64, ptr, ptr, ptr, ptr, ptr, ptr]),
    "fitgnn_louvain_components_workspace_bytes": (c_size, [c_i64]),
    "fitgnn_louvain_components": (ctypes.c_int, [ptr, ptr, c_i64, ptr, ptr, ptr, ptr, c_size, ptr]),
}

_lib = None
_plans = {}      # name -> per-parameter plan of call(), built once by lib()
_Tensor = None   # torch.Tensor, set by lib()
_NO_CPU = "fitgnn ops run on the MI355X only: got a CPU tensor (no CPU fallback exists)"


class FitgnnError(RuntimeError):
    pass


def _plan(argtypes):
    """(number of parameters, positions of the pointers, (position, lo, hi) of every integer parameter: the range of its type) of one
    signature; what ctypes converts alone (floats) is in neither list."""
    ints = []
    for i, t in enumerate(argtypes):
        if t in (c_i32, c_u32, c_i64, c_u64, c_size):
            bits, signed = 8 * ctypes.sizeof(t), t(-1).value < 0
            ints.append((i, -(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (i, 0, (1 << bits) - 1))
    return len(argtypes), tuple(i for i, t in enumerate(argtypes) if t is ptr), tuple(ints)


def lib():
    """The loaded library; raises (never falls back) when it is not built."""
    global _lib, _Tensor
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FitgnnError(f"{LIB_PATH} not found: build the HIP extension first "
                              "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        # torch first: its wheel carries its own HIP runtime, and the process must hold ONE -- the library's libamdhip64
        # dependency then resolves to the copy torch has loaded.  Loaded the other way round (library first, e.g. build()
        # followed by smoke() in one process) the two runtimes coexist and this library's sees no device (hipErrorNoDevice).
        import torch  # noqa: F401

        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
            _plans[name] = _plan(args)
        if L.fitgnn_abi_version() != 1:
            raise FitgnnError("libfitgnn_hip.so ABI version mismatch")
        _Tensor = torch.Tensor
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().fitgnn_error_string(int(rc)).decode()
        raise FitgnnError(f"{what}: {msg} (code {rc})")


def call(name, *args):
    """Call the status-returning entry point `name` (a key of SIGNATURES) and raise FitgnnError unless it returns 0.

    Each argument is converted by its parameter's declared type before anything is launched.  A pointer takes a CUDA tensor (its
    data_ptr(); a CPU tensor is an error: there is no CPU fallback), None (NULL), or anything ctypes itself takes for a void*
    (an int address, a c_void_p, a ctypes array, a byref).  An integer must fit the parameter's type: ctypes would truncate it
    silently.  The stream is an argument like any other."""
    L = _lib or lib()   # the library object of this moment: a tool may have put a wrapper in its place
    try:
        n, ptrs, ints = _plans[name]
    except KeyError:
        raise FitgnnError(f"{name}: not an entry point that lib() has bound (SIGNATURES lists them)") from None
    if len(args) != n:
        raise FitgnnError(f"{name}: takes {n} arguments, got {len(args)}")
    for i, lo, hi in ints:
        if not lo <= args[i] <= hi:
            raise FitgnnError(f"{name}: argument {i} = {args[i]} does not fit {SIGNATURES[name][1][i].__name__}")
    conv = list(args)
    for i in ptrs:
        a = conv[i]
        if a is not None and isinstance(a, _Tensor):   # (None first: an identity test costs less than isinstance)
            if not a.is_cuda:
                raise FitgnnError(_NO_CPU)
            conv[i] = a.data_ptr()
    rc = getattr(L, name)(*conv)
    if rc:
        check(rc, name)


def dptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FitgnnError(_NO_CPU)
