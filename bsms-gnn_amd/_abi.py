"""ctypes binding of libbsms_hip.so (include/bsms_hip.h).  No torch types cross this boundary: only
raw device pointers, sizes and the HIP stream handle.  There is NO CPU fallback: if the library is
missing or a call fails, this raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbsms_hip.so")

c_i64, c_int, c_void_p, c_size_t = C.c_int64, C.c_int, C.c_void_p, C.c_size_t
PP = C.POINTER(c_void_p)

# name -> (restype, argtypes); one entry per declaration in include/bsms_hip.h
SIGNATURES = {
    "bsms_abi_version": (c_int, []),
    "bsms_last_error": (C.c_char_p, []),
    "bsms_plan_create": (c_int, [c_void_p, c_i64, c_i64, PP]),
    "bsms_plan_set_pool": (c_int, [c_void_p, c_void_p, c_i64]),
    "bsms_plan_bind_edge_weights": (c_int, [c_void_p, c_void_p, c_void_p]),
    "bsms_plan_bound_edge_weights": (c_void_p, [c_void_p]),
    "bsms_plan_destroy": (c_int, [c_void_p]),
    "bsms_plan_pool_trim": (c_int, []),
    "bsms_plan_num_nodes": (c_i64, [c_void_p]),
    "bsms_plan_num_edges": (c_i64, [c_void_p]),
    "bsms_plan_num_pooled": (c_i64, [c_void_p]),
    "bsms_plan_min_out_degree": (c_i64, [c_void_p]),
    "bsms_plan_max_source": (c_i64, [c_void_p]),
    "bsms_plan_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_plan_export_ex": (c_i64, [c_void_p, c_int, c_void_p]),
    "bsms_plan_concat": (c_int, [PP, c_int, c_void_p, c_void_p, c_void_p, c_void_p, PP]),
    "bsms_segment_sum_fwd": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p]),
    "bsms_segment_sum_bwd": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p]),
    "bsms_segment_sum_bf16": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p]),
    "bsms_cal_ew": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_edge_conv": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "bsms_scatter_rows": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p]),
    "bsms_gather_rows": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p]),
    "bsms_mlp_saved_bytes": (c_size_t, [c_i64, c_i64, c_i64, c_i64, c_int]),
    "bsms_mlp_work_bytes": (c_size_t, [c_i64, c_i64, c_i64, c_i64, c_int]),
    "bsms_mlp_fwd": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, PP, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_mlp_fwd_ex": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, PP, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "bsms_pack_group_create": (c_int, [PP]),
    "bsms_pack_group_destroy": (None, [c_void_p]),
    "bsms_pack_group_add_mlp": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, PP, c_void_p, c_void_p]),
    "bsms_pack_group_add_bsgmp": (c_int, [c_void_p, PP, c_int, c_i64, c_i64, c_i64, c_int, PP, c_void_p, c_void_p, c_int]),
    "bsms_pack_group_launch": (c_int, [c_void_p, c_void_p]),
    "bsms_mlp_bwd": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, PP, c_void_p, c_void_p,
                             c_void_p, PP, c_void_p]),
    "bsms_mlp_bwd_ex": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, c_int, PP, c_void_p, c_void_p,
                                c_void_p, PP, c_int, c_void_p]),
    "bsms_gmp_saved_bytes": (c_size_t, [c_i64, c_i64, c_i64, c_i64, c_int]),
    "bsms_gmp_work_bytes": (c_size_t, [c_i64, c_i64, c_i64, c_i64, c_int]),
    "bsms_gmp_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
    "bsms_gmp_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                             c_void_p, c_void_p, PP, c_void_p]),
    "bsms_gmp_pos_work_bytes": (c_size_t, [c_i64, c_i64, c_i64]),
    "bsms_gmp_bwd_pos": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                 c_void_p, c_void_p, PP, c_void_p, c_void_p, c_void_p]),
    "bsms_bsgmp_saved_bytes": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int]),
    "bsms_bsgmp_work_bytes": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int]),
    "bsms_bsgmp_infer_work_bytes": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int]),
    "bsms_bsgmp_fwd": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "bsms_bsgmp_fwd_ex": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p, c_void_p,
                                  c_void_p, c_int, c_void_p]),
    "bsms_bsgmp_saved_bytes_p": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int, c_int]),
    "bsms_bsgmp_saved_bytes_ex": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int]),
    "bsms_bsgmp_work_bytes_ex": (c_size_t, [PP, c_int, c_i64, c_i64, c_i64, c_int, c_int, c_int]),
    "bsms_bsgmp_fwd_p": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p, c_void_p,
                                 c_void_p, c_int, c_int, c_void_p]),
    "bsms_bsgmp_bwd_p": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                 c_void_p, c_void_p, PP, c_int, c_void_p]),
    "bsms_bsgmp_bwd": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                               c_void_p, c_void_p, PP, c_void_p]),
    "bsms_bsgmp_bwd_ex": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                  c_void_p, c_void_p, PP, c_int, c_int, c_void_p]),
    "bsms_bsgmp_bwd_ev": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                  c_void_p, c_void_p, PP, c_int, c_int, PP, c_void_p]),
    "bsms_bsgmp_pos_work_bytes": (c_size_t, [PP, c_int, c_i64, c_i64]),
    "bsms_bsgmp_bwd_pos": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                   c_void_p, c_void_p, PP, c_int, c_void_p, c_void_p, c_void_p]),
    "bsms_bsgmp_bwd_pos_ev": (c_int, [PP, PP, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_int, PP, c_void_p,
                                      c_void_p, c_void_p, PP, c_int, c_int, PP, c_void_p, c_void_p, c_void_p]),
    "bsms_side_lanes_join": (c_int, [c_void_p]),
    "bsms_streams_overlap": (c_int, [c_void_p, c_void_p]),
    "bsms_sim_work_bytes": (c_size_t, [c_i64]),
    "bsms_sim_prologue": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_sim_epilogue": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_sim_loss_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "bsms_sim_unroll_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_sim_objective_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_int, c_int, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "bsms_sim_objective_bwd_w": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, C.c_float, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_sim_robust_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, C.c_float, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_sim_input_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p,
                                    c_int, c_int, c_void_p, c_void_p]),
    "bsms_error_sums_work_bytes": (c_size_t, [c_i64, c_i64]),
    "bsms_error_sums": (c_int, [c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
    "bsms_error_sums_w": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p,
                                  c_void_p, c_void_p]),
    "bsms_robust_sums": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_i64, c_void_p, c_void_p]),
    "bsms_edge_diff_work_bytes": (c_size_t, [c_i64, c_i64]),
    "bsms_edge_diff_sums": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_i64,
                                    c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
    "bsms_edge_diff_bwd": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_i64, c_int, c_i64,
                                   c_i64, c_i64, c_i64, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
    "bsms_batch_assemble": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, C.c_double, c_void_p, c_i64, C.c_uint64, C.c_uint64,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_batch_targets": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p]),
    "bsms_batch_assemble_xf": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_i64, c_void_p, C.c_double, c_void_p, c_i64,
                                       C.c_uint64, C.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_rows_transform": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_int, c_void_p, c_i64,
                                    c_void_p]),
    "bsms_hierarchy_create": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, PP]),
    "bsms_hierarchy_create_f32": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, PP]),
    "bsms_hierarchy_destroy": (c_int, [c_void_p]),
    "bsms_hierarchy_level_nodes": (c_i64, [c_void_p, c_int]),
    "bsms_hierarchy_level_edges": (c_i64, [c_void_p, c_int]),
    "bsms_hierarchy_copy_edges": (c_int, [c_void_p, c_int, c_void_p]),
    "bsms_hierarchy_copy_ids": (c_int, [c_void_p, c_int, c_void_p]),
    "bsms_adamw_work_bytes": (c_size_t, []),
    "bsms_adamw_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_float, c_i64, C.c_float, c_void_p, c_void_p, c_void_p]),
    "bsms_optim_groups_create": (c_int, [c_void_p, c_int, c_i64, PP]),
    "bsms_optim_groups_destroy": (c_int, [c_void_p]),
    "bsms_optim_work_bytes": (c_size_t, []),
    "bsms_optim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, C.c_float, C.c_float, C.c_float, C.c_float,
                                C.c_float, c_i64, C.c_float, c_void_p, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_grad_accumulate": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p]),
    "bsms_accum_coef": (c_int, [c_void_p, c_int, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_i64, c_i64,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "bsms_grad_fold": (c_int, [c_void_p, c_void_p, c_i64, c_void_p, c_void_p]),
    "bsms_wgrad_bound_width": (c_size_t, []),
    "bsms_wgrad_work_bytes": (c_size_t, [c_i64, c_int]),
    "bsms_wgrad": (c_int, [c_void_p, c_int, c_i64, C.c_uint, c_void_p, c_size_t, c_void_p]),
    "bsms_small_wgrad_work_bytes": (c_size_t, [c_i64]),
    "bsms_small_wgrad": (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_void_p, c_i64, c_i64, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]),
}


# the companion library libbsms_hip_ext.so: name -> (restype, argtypes); one entry per declaration in include/bsms_hip_ext.h
EXT_LIB_PATH = os.path.join(_HERE, "libbsms_hip_ext.so")
EXT_SIGNATURES = {
    "bsms_edge_diff_fold": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_void_p]),
    "bsms_sim_edge_objective_bwd": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                            C.c_double, C.c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
}


# the second companion library libbsms_hip_stats.so: name -> (restype, argtypes); one entry per declaration in include/bsms_hip_stats.h
STATS_LIB_PATH = os.path.join(_HERE, "libbsms_hip_stats.so")
STATS_SIGNATURES = {
    "bsms_moment_work_bytes": (c_size_t, [c_i64]),
    "bsms_moment_sums": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_void_p]),
    "bsms_moment_fold": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_void_p]),
}


# the third companion library libbsms_hip_sample.so: name -> (restype, argtypes); one entry per declaration in include/bsms_hip_sample.h
SAMPLE_LIB_PATH = os.path.join(_HERE, "libbsms_hip_sample.so")
SAMPLE_SIGNATURES = {
    "bsms_raster_work_bytes": (c_size_t, []),
    "bsms_raster_owner": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_i64, C.c_double, C.c_double, C.c_double, C.c_double, c_i64,
                                  c_void_p, c_void_p, c_void_p]),
    "bsms_point_owner": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_void_p, c_void_p]),
    "bsms_field_gather": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_i64, c_i64, C.c_double, C.c_double,
                                  C.c_double, C.c_double, c_void_p, c_i64, c_i64, c_i64, c_i64, C.c_float, c_void_p, c_void_p]),
}


# the fourth companion library libbsms_hip_query.so: name -> (restype, argtypes); one entry per declaration in include/bsms_hip_query.h
QUERY_LIB_PATH = os.path.join(_HERE, "libbsms_hip_query.so")
QUERY_SIGNATURES = {
    "bsms_chain_launch_query": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
}


# the fifth companion library libbsms_hip_diffop.so: name -> (restype, argtypes); one entry per declaration in include/bsms_hip_diffop.h
DIFFOP_LIB_PATH = os.path.join(_HERE, "libbsms_hip_diffop.so")
DIFFOP_SIGNATURES = {
    "bsms_cell_gradient": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_i64, C.c_float, c_void_p, c_void_p]),
    "bsms_node_gradient": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_i64, c_i64,
                                   C.c_float, c_i64, c_void_p, c_void_p]),
    "bsms_cell_gradient_work_bytes": (c_size_t, [c_i64, c_i64]),
    "bsms_cell_gradient_sums": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                        c_i64, c_i64, c_i64, c_i64, c_void_p, c_void_p, c_void_p]),
    "bsms_cell_gradient_bwd": (c_int, [c_void_p, c_i64, c_i64, c_void_p, c_i64, c_void_p, c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_i64,
                                       c_i64, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_void_p, c_int, c_void_p, c_i64, c_void_p]),
}


class MomentTraj(C.Structure):
    """bsms_moment_traj (include/bsms_hip_stats.h)."""
    _fields_ = [("state", c_void_p), ("type", c_void_p), ("n", c_i64), ("frame0", c_i64), ("frames", c_i64), ("type_stride", c_i64)]


class ChainLaunchKey(C.Structure):
    """bsms_chain_launch_key (include/bsms_hip_query.h)."""
    _fields_ = [("R", c_i64), ("nstage", c_int), ("nseq", c_int), ("bf16", c_int), ("store_mode", c_int), ("timing", c_int),
                ("resid", c_int), ("act_stores", c_int), ("glast", c_int), ("gstores", c_int), ("masks", c_int)]


class ChainLaunchInfo(C.Structure):
    """bsms_chain_launch_info (include/bsms_hip_query.h)."""
    _fields_ = [("family", c_int), ("rb", c_int), ("save", c_int), ("store", c_int), ("lone", c_int), ("bf16", c_int), ("timing", c_int),
                ("cw", c_int), ("nload", c_int), ("nring", c_int), ("ntiles", c_int), ("grid", c_i64), ("threads", c_i64), ("lds", c_i64),
                ("lds_max", c_i64), ("name", C.c_char * 48)]


class WgradJob(C.Structure):
    """bsms_wgrad_job (include/bsms_hip.h)."""
    _fields_ = [("G", c_void_p), ("A", c_void_p), ("dW", c_void_p), ("db", c_void_p), ("R", c_i64),
                ("ldg", c_int), ("lda", c_int), ("ldw", c_int), ("col0", c_int), ("bf16", c_int),
                ("g_bound", c_void_p), ("a_bound", c_void_p), ("g_mul", C.c_float), ("a_mul", C.c_float)]


class OptimGroup(C.Structure):
    """bsms_optim_group_t (include/bsms_hip.h)."""
    _fields_ = [("offset", c_i64), ("count", c_i64), ("lr_scale", C.c_float), ("weight_decay", C.c_float)]


_ERRORS = {-1: "BSMS_E_INVALID_ARG", -2: "BSMS_E_SHAPE", -3: "BSMS_E_UNSUPPORTED", -4: "BSMS_E_HIP"}
_lib = None


class BsmsError(RuntimeError):
    pass


def lib():
    """Load the shared library (once).  Raises if it has not been built -- the product path never
    silently degrades to a PyTorch implementation."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BsmsError(f"{LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` "
                            "(or __graft_entry__.build()); there is no CPU/PyTorch fallback")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


_ext = None


def ext():
    """Load the companion library (once), behind libbsms_hip.so, which it links against.  Raises if it has not been built."""
    global _ext
    if _ext is None:
        lib()
        if not os.path.exists(EXT_LIB_PATH):
            raise BsmsError(f"{EXT_LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` (or __graft_entry__.build()); "
                            "there is no CPU/PyTorch fallback")
        handle = C.CDLL(EXT_LIB_PATH)
        for name, (res, args) in EXT_SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _ext = handle
    return _ext


_stats = None


def stats():
    """Load the statistics library (once), behind libbsms_hip.so, which it links against.  Raises if it has not been built.  Only the
    dataset statistics (ops.moment_sums / moment_fold) call this: a process that never asks for them never loads the library."""
    global _stats
    if _stats is None:
        lib()
        if not os.path.exists(STATS_LIB_PATH):
            raise BsmsError(f"{STATS_LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` (or __graft_entry__.build()); "
                            "there is no CPU/PyTorch fallback")
        handle = C.CDLL(STATS_LIB_PATH)
        for name, (res, args) in STATS_SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _stats = handle
    return _stats


_sample = None


def sample():
    """Load the sampling library (once), behind libbsms_hip.so, which it links against.  Raises if it has not been built.  Only the
    mesh sampler (sample.MeshSampler) calls this: a process that never samples a field never loads the library."""
    global _sample
    if _sample is None:
        lib()
        if not os.path.exists(SAMPLE_LIB_PATH):
            raise BsmsError(f"{SAMPLE_LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` (or __graft_entry__.build()); "
                            "there is no CPU/PyTorch fallback")
        handle = C.CDLL(SAMPLE_LIB_PATH)
        for name, (res, args) in SAMPLE_SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _sample = handle
    return _sample


_query = None


def query():
    """Load the query library (once), behind libbsms_hip.so, which it links against.  Raises if it has not been built.  For tests and
    tools: nothing on the product path calls this."""
    global _query
    if _query is None:
        lib()
        if not os.path.exists(QUERY_LIB_PATH):
            raise BsmsError(f"{QUERY_LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` (or __graft_entry__.build()); "
                            "there is no CPU/PyTorch fallback")
        handle = C.CDLL(QUERY_LIB_PATH)
        for name, (res, args) in QUERY_SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _query = handle
    return _query


_diffop = None


def diffop():
    """Load the differential-operator library (once), behind libbsms_hip.so, which it links against.  Raises if it has not been built.
    Only the mesh gradients (diffop.MeshGradient) call this: a process that never differentiates a field never loads the library."""
    global _diffop
    if _diffop is None:
        lib()
        if not os.path.exists(DIFFOP_LIB_PATH):
            raise BsmsError(f"{DIFFOP_LIB_PATH} not found: build it with `python bsms-gnn_amd/build.py` (or __graft_entry__.build()); "
                            "there is no CPU/PyTorch fallback")
        handle = C.CDLL(DIFFOP_LIB_PATH)
        for name, (res, args) in DIFFOP_SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _diffop = handle
    return _diffop


def check(rc, what):
    if rc != 0:
        msg = lib().bsms_last_error().decode(errors="replace")
        raise BsmsError(f"{what}: {_ERRORS.get(rc, rc)}: {msg}")


def ptr_array(ptrs):
    arr = (c_void_p * len(ptrs))(*ptrs)
    return C.cast(arr, PP), arr  # keep `arr` alive while the call runs
