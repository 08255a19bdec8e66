"""ctypes binding of libcsx.so (include/csx.h).  Thin on purpose: prototypes,
status -> exception mapping, numpy <-> pointer helpers.  There is no CPU
fallback: if the HIP library or a GPU is missing, calls raise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CSX_LIB: load another build of the library (the -DCSX_ABLATION build used for the timing experiments)
LIB_PATH = os.environ.get("CSX_LIB") or os.path.join(_HERE, "libcsx.so")

OK, EINVAL, EZEROPIVOT, ENOTSPD, ERUNTIME = 0, 1, 2, 3, 4
TRI_L, TRI_LT, TRI_U, TRI_UT = 0, 1, 2, 3
GAXPY_AUTO, GAXPY_EXACT, GAXPY_WAVE, GAXPY_TILED, GAXPY_ATOMIC = 0, 1, 2, 3, 4

H = C.c_uint64
_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p

_PROTOS = {
    "csx_init": [C.c_int],
    "csx_finalize": [],
    "csx_sync": [],
    "csx_set_stream": [_vp],
    "csx_device_info": [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)],
    "csx_compress": [C.c_int32, C.c_int32, C.c_int64, _i32p, _i32p, _f64p, C.POINTER(H)],
    "csx_add": [H, H, C.c_double, C.c_double, C.POINTER(H)],
    "csx_dupl": [H, C.POINTER(H)],
    "csx_drop": [H, C.c_int, C.c_double, C.POINTER(H)],
    "csx_permute": [H, _i32p, _i32p, C.c_int, C.POINTER(H)],
    "csx_symperm": [H, _i32p, C.c_int, C.POINTER(H)],
    "csx_schol": [H, _i32p, _i32p],
    "csx_order_nd_host": [C.c_int32, _i32p, _i32p, _i32p],
    "csx_norm1": [H, _f64p],
    "csx_cholsol_set_order": [H, C.c_int],
    "csx_cholsol_growth": [H, _f64p],
    "csx_cholsol_sn_info": [H, _i32p, _i32p, _i32p, _i32p, _f64p],
    "csx_cholsol_sn_geometry": [H, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_cholsol_sn_launches": [H, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_csc_invalidate": [H],
    "csx_set_option": [C.c_char_p, C.c_int],
    "csx_get_option": [C.c_char_p, C.POINTER(C.c_int)],
    "csx_gaxpy_host": [C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _f64p, _f64p],
    "csx_csc_col_block": [H, C.c_int32, C.c_int32, C.POINTER(H)],
    "csx_mem_trim": [],
    "csx_mem_info": [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "csx_timer_start": [],
    "csx_timer_stop": [_f64p],
    "csx_csc_upload": [C.c_int32, C.c_int32, _i32p, _i32p, _f64p, C.POINTER(H)],
    "csx_csc_alloc": [C.c_int32, C.c_int32, C.c_int32, C.c_int, C.POINTER(H)],
    "csx_csc_wrap": [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.POINTER(H)],
    "csx_csc_info": [H, _i32p, _i32p, _i32p, C.POINTER(C.c_int)],
    "csx_csc_download": [H, _i32p, _i32p, _f64p],
    "csx_csc_ptrs": [H, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
    "csx_free": [H],
    "csx_vec_alloc": [C.c_int64, C.POINTER(H)],
    "csx_vec_upload": [_f64p, C.c_int64, C.POINTER(H)],
    "csx_vec_wrap": [_vp, C.c_int64, C.POINTER(H)],
    "csx_vec_download": [H, _f64p, C.c_int64],
    "csx_vec_write": [H, _f64p, C.c_int64],
    "csx_vec_fill": [H, C.c_double],
    "csx_vec_copy": [H, H],
    "csx_vec_ptr": [H, C.POINTER(_vp), C.POINTER(C.c_int64)],
    "csx_ivec_upload": [_i32p, C.c_int64, C.POINTER(H)],
    "csx_ivec_download": [H, _i32p, C.c_int64],
    "csx_gaxpy": [H, H, H, C.c_int],
    "csx_gaxpy_prepare": [H, C.c_int],
    "csx_gaxpy_block": [H, H, H, C.c_int32, C.c_int],
    "csx_residual_block": [H, H, H, H, C.c_int32, C.c_int, _f64p, _f64p],
    "csx_residual_host": [C.c_int32, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, C.c_int, _f64p, _f64p, _f64p, _f64p, _f64p],
    "csx_residual_sym_block": [H, H, H, H, C.c_int32, _f64p, _f64p],
    "csx_residual_sym_host": [C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p],
    "csx_norm1_sym": [H, _f64p],
    "csx_block_add_cols": [H, H, H, C.c_int64, C.c_int32, _i32p],
    "csx_block_select_cols": [H, H, C.c_int64, C.c_int32, _i32p],
    "csx_transpose": [H, C.c_int, C.POINTER(H)],
    "csx_cumsum": [H, H, C.c_int64, C.POINTER(C.c_int64)],
    "csx_prim_limits": [_i32p],
    "csx_prim_scan": [_i32p, _i32p, C.c_int64, C.c_int, C.POINTER(C.c_int64)],
    "csx_prim_suffix_min": [_i32p, C.c_int64],
    "csx_prim_expand_columns": [_i32p, C.c_int32, C.c_int32, _i32p],
    "csx_prim_boundaries": [_vp, C.c_int64, C.c_int32, _i32p, C.c_int],
    "csx_prim_sort": [_vp, _vp, _f64p, C.c_int64, C.c_uint32, _vp, _vp, _f64p, _i32p, C.c_int32, _i32p, C.c_int32, C.c_int],
    "csx_prim_sort_info": [C.POINTER(C.c_int64), C.c_int32],
    "csx_multiply": [H, H, C.POINTER(H)],
    "csx_spgemm_limits": [_i32p],
    "csx_spgemm_info": [C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_tri_analyse": [H, C.c_int, C.POINTER(H)],
    "csx_tri_info": [H, _i32p, _i32p, _i32p],
    "csx_tri_solve": [H, H, C.c_int32],
    "csx_tri_set_order": [H, C.c_int],
    "csx_tri_solve_list": [H, _f64p, C.POINTER(C.c_int)],
    "csx_cholsol_solve_list": [H, _f64p, C.POINTER(C.c_int)],
    "csx_tri_order_info": [H, _i32p, _f64p],
    "csx_tri_components": [H, _i32p],
    "csx_tri_limits": [_i32p],
    "csx_tri_route_info": [H, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_tri_launches": [H, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_cholsol_tri_route_info": [H, C.c_int, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_cholsol_tri_launches": [H, C.c_int, C.POINTER(C.c_int64), C.c_int32, _i32p],
    "csx_permute_vec": [H, H, H, C.c_int32, C.c_int32, C.c_int],
    "csx_lusol_solve": [H, H, H, H, H, H, C.c_int32, C.POINTER(C.c_int)],
    "csx_lusol_solve_trans": [H, H, H, H, H, H, C.c_int32, C.POINTER(C.c_int)],
    "csx_schol_host": [C.c_int32, _i32p, _i32p, _i32p, _i32p],
    "csx_counts_host": [C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, C.c_int, _i32p],
    "csx_chol": [H, _i32p, _i32p, _i32p, C.POINTER(H)],
    "csx_chol_info": [_i32p, _f64p],
    "csx_cholsol_plan": [H, _i32p, C.POINTER(H)],
    "csx_cholsol_factor": [H, C.c_int, C.POINTER(H), C.POINTER(H)],
    "csx_cholsol_factor_info": [C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "csx_cholsol_solve": [H, H, C.c_int32],
    "csx_cholsol_graph_info": [H, _i32p, _f64p],
    "csx_cholsol_info": [H, _i32p, _i32p, _i32p],
    "csx_qr_host": [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                    _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, _f64p],
    "csx_qr_apply_host": [C.c_int32, _i32p, _i32p, _f64p, _f64p, C.c_int, _f64p],
    "csx_lu_blocks": [H, C.c_double, C.POINTER(H), C.POINTER(H), _i32p, C.POINTER(C.c_int)],
    "csx_block_limits": [_i32p],
    "csx_prim_components": [C.c_int32, _i32p, _i32p, C.c_int, C.c_int, C.c_int, _i32p, _vp, _i32p, _i32p, _i32p, _i32p, _i32p,
                            C.POINTER(C.c_int)],
    "csx_lu_etree": [H, C.c_double, C.POINTER(H), C.POINTER(H), _i32p, C.POINTER(C.c_int)],
    "csx_updown": [H, C.c_int, C.c_int32, _i32p, _f64p, _i32p, C.POINTER(C.c_int)],
    "csx_updown_block": [H, H, _i32p, _i32p, C.c_int, _i32p],
    "csx_updown_block_info": [_i32p, _i32p, _i32p, _f64p],
    "csx_updown_block_classes": [_i32p, _i32p],
    "csx_chol_inverse": [H, C.POINTER(H)],
    "csx_chol_inverse_info": [_i32p, _i32p, C.POINTER(C.c_int64), _f64p],
    "csx_csc_diag": [H, H],
    "csx_ldl_inverse": [H, H, C.POINTER(H)],
    "csx_slu_inverse": [H, H, C.POINTER(H), C.POINTER(H)],
    "csx_inverse_at": [H, H, H, H, C.c_int64, _i32p, _i32p, H, C.POINTER(C.c_int64)],
    "csx_spsolve": [H, H, _i32p, C.c_int, C.c_int, C.POINTER(H)],
    "csx_happly": [H, H, H, C.c_int32, C.c_int],
    "csx_sqr_host": [C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_int32),
                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "csx_qr_blocks": [H, _i32p, _i32p, _i32p, C.c_int32, C.POINTER(H), C.POINTER(H), _f64p, C.POINTER(C.c_int)],
    "csx_gaxpy_plan_info": [H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "csx_gaxpy_plan_shape": [H, C.POINTER(C.c_int), C.POINTER(C.c_double)],
    "csx_gaxpy_plan_geometry": [H, C.POINTER(C.c_int64)],
    "csx_gaxpy_plan_groups": [H, _i32p],
    "csx_lu_host": [C.c_int32, _i32p, _i32p, _f64p, C.c_double, C.POINTER(_i32p), C.POINTER(_i32p),
                    C.POINTER(_f64p), C.POINTER(_i32p), C.POINTER(_i32p), C.POINTER(_f64p), _i32p],
    "csx_comm_unique_id": [C.POINTER(C.c_uint8)],
    "csx_comm_init": [C.c_int, C.c_int, C.POINTER(C.c_uint8)],
    "csx_comm_finalize": [],
    "csx_comm_info": [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "csx_comm_barrier": [],
    "csx_comm_allreduce_host": [_f64p, C.c_int, C.c_int],
    "csx_comm_bcast_host": [_vp, C.c_int64, C.c_int],
    "csx_comm_bcast_csc": [C.POINTER(H), C.c_int],
    "csx_comm_bcast_vec": [H, C.c_int],
    "csx_comm_reduce_scatter_vec": [H, H],
    "csx_comm_allreduce_vec": [H],
    "csx_comm_scatter_blocks": [H, H, C.c_int64, C.c_int],
    "csx_comm_gather_blocks": [H, H, C.c_int64, C.c_int],
    "csx_block_cols": [H, C.c_int64, C.c_int32, C.c_int32, C.c_int32, H, C.c_int],
    "csx_gaxpy_sharded_plan": [H, C.POINTER(H)],
    "csx_gaxpy_sharded_rows": [H, _i32p, _i32p],
    "csx_gaxpy_sharded": [H, H, H, C.c_int],
    "csx_gaxpy_sharded_plan_for": [H, C.c_int, C.POINTER(H)],
    "csx_gaxpy_sharded_piece": [H, C.c_int, H],
    "csx_gaxpy_sharded_buffers": [H, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64)],
    "csx_gaxpy_sharded_sum": [H, C.c_int, C.c_int, H],
    "csx_maxtrans": [H, C.c_int64, _i32p, _i32p],
    "csx_scc": [H, _i32p, _i32p, _i32p],
    "csx_dmperm": [H, C.c_int64, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p],
    "csx_dmperm_times": [_f64p],
    "csx_dmperm_rounds": [C.POINTER(C.c_int64)],
    "csx_btf_split": [H, _i32p, _i32p, _i32p, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, C.POINTER(H), C.POINTER(H)],
    "csx_btf_plan": [H, H, H, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.POINTER(H)],
    "csx_btf_solve": [H, H, H, C.c_int32],
    "csx_btf_solve_trans": [H, H, H, C.c_int32],
    "csx_btf_info": [H, C.POINTER(C.c_int64)],
    "csx_btf_limits": [_i32p],
    "csx_btf_refactor": [H, H, H, H, C.POINTER(C.c_int), _f64p, C.POINTER(C.c_int64)],
    "csx_btf_refactor_dx": [H, _f64p],
    "csx_lu_refactor_plan": [H, H, H, _i32p, _i32p, C.POINTER(H)],
    "csx_lu_refactor": [H, H, C.POINTER(C.c_int), _f64p, C.POINTER(C.c_int64)],
    "csx_chol_refactor_plan": [H, H, _i32p, C.POINTER(H)],
    "csx_chol_refactor": [H, H, C.POINTER(C.c_int), _i32p],
    "csx_chol_refactor_info": [C.POINTER(C.c_double), C.POINTER(C.c_double)],
    "csx_chol_refactor_window": [H, C.POINTER(C.c_int32)],
    "csx_chol_limits": [_i32p],
    "csx_cholsol_forest_plan": [C.c_int, C.c_int32, C.c_int32, C.c_int, C.c_int, C.POINTER(C.c_int32)],
    "csx_lu_refactor_host": [C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _f64p, _i32p, _i32p, _f64p,
                             C.POINTER(C.c_int), _f64p],
    "csx_assemble_plan_host": [C.c_int32, C.c_int32, C.c_int64, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p],
    "csx_assemble_host": [C.c_int32, _i32p, _i32p, _f64p, _f64p],
    "csx_assemble_plan": [C.c_int32, C.c_int32, C.c_int64, _i32p, _i32p, C.POINTER(H)],
    "csx_assemble_matrix": [H, H, C.POINTER(H)],
    "csx_assemble": [H, H, H],
    "csx_assemble_plan_info": [H, C.POINTER(C.c_int64)],
    "csx_assemble_pullback": [H, H, H],
    "csx_assemble_pullback_host": [C.c_int32, C.c_int64, _i32p, _i32p, _f64p, _f64p],
    "csx_pattern_outer": [H, H, H, C.c_int32, C.c_int, C.c_double, H],
    "csx_pattern_outer_host": [C.c_int32, C.c_int32, _i32p, _i32p, C.c_int32, C.c_int, C.c_double, _f64p, _f64p, _f64p],
    "csx_pattern_outer_limits": [C.POINTER(C.c_int64)],
    "csx_multiply_plan_count": [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_int64),
                                C.POINTER(C.c_int64)],
    "csx_multiply_plan_host": [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p],
    "csx_multiply_fold_host": [C.c_int32, _i32p, _i32p, _f64p, _f64p, _f64p],
    "csx_multiply_plan": [H, H, C.POINTER(H)],
    "csx_multiply_plan_matrix": [H, H, H, H, C.POINTER(H)],
    "csx_multiply_plan_run": [H, H, H, H, H],
    "csx_multiply_plan_info": [H, C.POINTER(C.c_int64)],
    "csx_add_plan_host": [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_i32p), C.POINTER(_i32p), _i32p, _i32p, _i32p, _i32p, _i32p],
    "csx_add_fold_host": [C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _f64p, C.POINTER(_f64p), _f64p],
    "csx_add_plan": [C.c_int32, C.POINTER(H), C.POINTER(H)],
    "csx_add_plan_matrix": [H, _f64p, C.POINTER(H), C.POINTER(H)],
    "csx_add_plan_run": [H, _f64p, C.POINTER(H), H],
    "csx_add_plan_info": [H, C.POINTER(C.c_int64)],
    "csx_ldl_factor": [H, _i32p, _i32p, _i32p, C.c_double, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_ldl_refactor": [H, H, C.c_double, C.POINTER(C.c_int)],
    "csx_ldl_parts": [H, C.POINTER(H), C.POINTER(H)],
    "csx_ldl_info": [H, C.POINTER(C.c_int64)],
    "csx_ldl_stats": [H, _f64p],
    "csx_ldl_window": [C.POINTER(C.c_int32)],
    "csx_block_div_rows": [H, H, C.c_int64, C.c_int32],
    "csx_ldl_host": [C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, C.c_double, _f64p, _f64p, C.POINTER(C.c_int64)],
    "csx_schur_factor": [H, _i32p, _i32p, _i32p, C.c_int32, C.c_double, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_schur_refactor": [H, H, C.c_double, C.POINTER(C.c_int)],
    "csx_schur_parts": [H, C.POINTER(H), C.POINTER(H), C.POINTER(H)],
    "csx_schur_info": [H, C.POINTER(C.c_int64)],
    "csx_schur_stats": [H, _f64p],
    "csx_schur_host": [C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, C.c_int32, C.c_double, _f64p, _f64p, _f64p,
                       C.POINTER(C.c_int64)],
    "csx_slu_factor": [H, _i32p, _i32p, _i32p, _i32p, C.c_double, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_slu_refactor": [H, H, C.c_double, C.POINTER(C.c_int)],
    "csx_slu_parts": [H, C.POINTER(H), C.POINTER(H)],
    "csx_slu_info": [H, C.POINTER(C.c_int64)],
    "csx_slu_stats": [H, _f64p],
    "csx_slu_window": [C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "csx_slu_host": [C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, C.c_double, _f64p, _f64p, C.POINTER(C.c_int64)],
    "csx_slu_batch_factor": [H, H, C.c_int32, _f64p, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_slu_batch_refactor": [H, H, _f64p, C.POINTER(C.c_int)],
    "csx_slu_batch_norm1": [H, H, C.c_int32, _f64p],
    "csx_slu_batch_solve": [H, H, C.c_int32, C.c_int],
    "csx_slu_batch_info": [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "csx_slu_batch_stats": [H, _f64p],
    "csx_slu_batch_member": [H, C.c_int32, _f64p, _f64p],
    "csx_slu_batch_limits": [_i32p],
    "csx_ldl_batch_factor": [H, H, C.c_int32, _f64p, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_ldl_batch_refactor": [H, H, _f64p, C.POINTER(C.c_int)],
    "csx_ldl_batch_norm1": [H, H, C.c_int32, _f64p],
    "csx_ldl_batch_solve": [H, H, C.c_int32],
    "csx_ldl_batch_info": [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "csx_ldl_batch_stats": [H, _f64p],
    "csx_ldl_batch_member": [H, C.c_int32, _f64p, _f64p],
    "csx_ldl_batch_d": [H, _f64p],
    "csx_ldl_batch_limits": [_i32p],
    "csx_hqr_symbolic_host": [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                              _i32p, _i32p, _i32p, _i32p],
    "csx_hqr_host": [C.c_int32, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32,
                     _i32p, _i32p, _f64p, _i32p, _i32p, _f64p, _f64p],
    "csx_hqr_factor": [H, _i32p, _i32p, _i32p, _i32p, C.c_int32, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_hqr_refactor": [H, H, C.POINTER(C.c_int)],
    "csx_hqr_parts": [H, C.POINTER(H), C.POINTER(H), C.POINTER(H)],
    "csx_hqr_info": [H, C.POINTER(C.c_int64)],
    "csx_hqr_stats": [H, _f64p],
    "csx_hqr_window": [C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    "csx_hqr_batch_factor": [H, H, C.c_int32, C.POINTER(H), C.POINTER(C.c_int)],
    "csx_hqr_batch_refactor": [H, H, C.POINTER(C.c_int)],
    "csx_hqr_batch_solve": [H, H, H, C.c_int32, C.c_int],
    "csx_hqr_batch_info": [H, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "csx_hqr_batch_stats": [H, _f64p],
    "csx_hqr_batch_member": [H, C.c_int32, _f64p, _f64p, _f64p],
    "csx_hqr_batch_r_diag": [H, _f64p],
    "csx_hqr_batch_limits": [_i32p],
    "csx_level_schedule": [C.c_int32, _i32p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int64, _i32p, C.POINTER(C.c_int32)],
    "csx_row_view": [C.c_int32, _i32p, _i32p, C.c_int, _i32p, _i32p, _i32p],
    "csx_gmres_limits": [_i32p],
    "csx_gs_work_len": [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)],
    "csx_gs_project": [H, C.c_int32, H, H, C.c_int64, C.c_int32, _i32p, C.c_int, _f64p],
    "csx_gs_update": [H, C.c_int32, H, H, C.c_int64, C.c_int32, _i32p, C.c_int, _f64p, _f64p],
    "csx_gs_scale": [H, H, C.c_int32, H, C.c_int64, C.c_int32, _i32p, _f64p],
    "csx_gs_combine": [H, C.c_int32, H, H, C.c_int64, C.c_int32, _i32p, _f64p, _i32p],
    "csx_gs_host": [C.c_int, C.c_int64, C.c_int32, C.c_int32, _f64p, _f64p, _i32p, C.c_int, _f64p, _i32p, _f64p],
    "csx_bgs_limits": [_i32p],
    "csx_bgs_work_len": [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)],
    "csx_bgs_gram": [H, C.c_int32, C.c_int32, H, C.c_int32, H, C.c_int64, C.c_int, _f64p],
    "csx_bgs_update": [H, C.c_int32, C.c_int32, H, C.c_int32, H, C.c_int64, _f64p],
    "csx_bgs_combine": [H, C.c_int32, C.c_int32, H, C.c_int32, H, C.c_int64, _f64p],
    "csx_bgs_host": [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, C.c_int, _f64p, _f64p],
    "csx_gen_grand": [C.c_int32, C.c_int32, C.c_uint64, C.POINTER(H)],
    "csx_gen_grand_uniform": [C.c_int32, C.c_int32, C.c_uint64, C.POINTER(H)],
    "csx_gen_gspd": [C.c_int32, C.c_int32, C.c_uint64, C.POINTER(H)],
    "csx_gen_vec": [C.c_int64, C.c_uint64, C.c_double, C.c_double, C.POINTER(H)],
    "csx_gen_rhs": [C.c_int32, C.c_int32, C.c_int32, C.POINTER(H)],
}

_lib = None
_ready = False


class CsxError(RuntimeError):
    pass


class NotPositiveDefinite(ArithmeticError):
    pass


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch bundles its own libamdhip64.so (same soname as /opt/rocm's).
    A process that uses both libcsx and torch on the device must have them on ONE runtime, or device pointers of one
    are foreign to the other.  Loading torch's copy by path BEFORE libcsx makes the dynamic loader satisfy libcsx's
    DT_NEEDED libamdhip64.so.7 with it, whatever order `import torch` and `_csx.load()` then come in.  Nothing is
    initialised and torch is not imported.
    Taken when CSX_SHARE_TORCH_HIP=1, or at WORLD_SIZE > 1 with the gloo stand-in as the transport
    (CSX_COMM_BACKEND=gloo: shard.Comm imports torch there).  The RCCL transport (the default at WORLD_SIZE > 1) has no
    torch in the process: libcsx, librccl and libamdhip64 all come from the ROCm installation, the combination
    tests/test_gpu_comm.py runs.  A torch that is already imported has already loaded its runtime, and libcsx then
    binds to it with no help."""
    import sys
    if "torch" in sys.modules:
        return "torch (already imported)"
    want = os.environ.get("CSX_SHARE_TORCH_HIP")
    if want == "0" or (want is None and (int(os.environ.get("WORLD_SIZE", "1")) <= 1
                                         or os.environ.get("CSX_COMM_BACKEND") != "gloo")):
        return None
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    C.CDLL(path, mode=C.RTLD_GLOBAL)
    return path


HIP_RUNTIME = None


def load():
    """dlopen libcsx.so and set prototypes (no GPU needed for this)."""
    global _lib, HIP_RUNTIME
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libcsx.so is not built: run `python csparse.py_amd/build.py` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        HIP_RUNTIME = _share_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, args in _PROTOS.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
        lib.csx_last_error.restype = C.c_char_p
        lib.csx_last_error.argtypes = []
        lib.csx_host_free.restype = None
        lib.csx_host_free.argtypes = [_vp]
        _lib = lib
    return _lib


def ldl_window():
    """entries of a column that the LDL' column kernels keep in LDS (csx_ldl.h LDL_ACC), asked of the library; no GPU needed"""
    out = C.c_int32(0)
    check(load().csx_ldl_window(C.byref(out)), "csx_ldl_window")
    return out.value


_CHOL_LIMITS = ("CH_ACC", "CH_NARROW", "CH_SMALL_TREE", "CD_MAX", "CC_ACC", "CC_MAP", "CC_RUN_MIN", "CC_RUN_MAX", "CC_WAVES",
                "SN_MIN_WIDTH")


def chol_limits():
    """the constants the general cs_chol numeric is cut by (csx_chol.hip), asked of the library; no GPU needed: a dict of
    CH_ACC, CH_NARROW, CH_SMALL_TREE, CD_MAX, CC_ACC, CC_MAP, CC_RUN_MIN, CC_RUN_MAX, CC_WAVES, SN_MIN_WIDTH, "windows" (the
    five register-window widths, ascending) and "max_need" (the largest half-bandwidth + 1 a register window takes)"""
    out = (C.c_int32 * 16)()
    check(load().csx_chol_limits(out), "csx_chol_limits")
    d = {name: int(out[k]) for k, name in enumerate(_CHOL_LIMITS)}
    d["windows"] = tuple(int(out[k]) for k in range(10, 15))
    d["max_need"] = int(out[15])
    return d


FOREST_PLAN_KINDS = ("General", "EmitEqual", "Programs", "BlockListExact", "EmitRagged", "BlockListLite")


def cholsol_forest_plan(sparse, min_bs, max_bs, exact, dense_blocks):
    """the kind of solve plan csx_cholsol_factor makes for a forest of blocks (a name of FOREST_PLAN_KINDS, include/csx.h:
    csx_cholsol_forest_plan), asked of the library; no GPU needed"""
    kind = C.c_int32(-1)
    check(load().csx_cholsol_forest_plan(int(sparse), min_bs, max_bs, int(exact), int(dense_blocks), C.byref(kind)),
          "csx_cholsol_forest_plan")
    return FOREST_PLAN_KINDS[kind.value]


def slu_window():
    """(entries of a column that the static-pivot LU column kernels keep in LDS, levels one launch of its walker takes)
    (csx_slu.hip SLU_ACC, csx_levelwalk.h WALK_RUN_LEVELS), asked of the library; no GPU needed"""
    a, b = C.c_int32(0), C.c_int32(0)
    check(load().csx_slu_window(C.byref(a), C.byref(b)), "csx_slu_window")
    return a.value, b.value


SLU_BATCH_LIMITS = ("MAX_MEMBERS", "WALK_WAVES", "SOLVE_THREADS", "SOLVE_FETCH", "RUN_WAVES", "RUN_FETCH")


def slu_batch_limits():
    """the constants by which a batch of static-pivot LU value sets cuts members, right-hand sides and grids (csx_slu_batch.hip,
    csx_levelwalk.h), asked of the library; no GPU needed: a dict of MAX_MEMBERS (the most members of a batch), WALK_WAVES (the
    widest level a walker takes), SOLVE_THREADS ((row, column) pairs a solve workgroup of a wide level takes, a thread each),
    SOLVE_FETCH (terms of a chain such a thread fetches together), RUN_WAVES ((row, right-hand side) pairs a solve walker takes
    at a time, a wave each), RUN_FETCH (terms of a chain such a wave fetches together)"""
    out = (C.c_int32 * len(SLU_BATCH_LIMITS))()
    check(load().csx_slu_batch_limits(out), "csx_slu_batch_limits")
    return {name: int(out[k]) for k, name in enumerate(SLU_BATCH_LIMITS)}


def ldl_batch_limits():
    """the constants by which a batch of LDL' value sets cuts members, right-hand sides and grids (csx_ldl_batch.hip on
    csx_levelwalk.h and csx_batchsolve.h), asked of the library; no GPU needed: slu_batch_limits()'s dict (SLU_BATCH_LIMITS), the
    level walk and the solve sweeps being the same code"""
    out = (C.c_int32 * len(SLU_BATCH_LIMITS))()
    check(load().csx_ldl_batch_limits(out), "csx_ldl_batch_limits")
    return {name: int(out[k]) for k, name in enumerate(SLU_BATCH_LIMITS)}


HQR_BATCH_LIMITS = SLU_BATCH_LIMITS + ("HAPPLY_LANES", "HAPPLY_MAX_LEVELS")


def hqr_batch_limits():
    """the constants by which a batch of Householder QR value sets cuts members, right-hand sides and grids (csx_hqr_batch.hip on
    csx_levelwalk.h and csx_batchsolve.h), asked of the library; no GPU needed: slu_batch_limits()'s dict, then HAPPLY_LANES (the
    columns of X a workgroup of the batched reflection kernels takes, a lane each) and HAPPLY_MAX_LEVELS (more reflection levels
    than that, or as many as reflections, and one launch walks them all: csx_happly's rule)"""
    out = (C.c_int32 * len(HQR_BATCH_LIMITS))()
    check(load().csx_hqr_batch_limits(out), "csx_hqr_batch_limits")
    return {name: int(out[k]) for k, name in enumerate(HQR_BATCH_LIMITS)}


def hqr_window():
    """(slots of a column that the Householder QR column kernels keep in LDS, levels one launch of its walker takes)
    (csx_hqr.hip HQR_ACC, csx_levelwalk.h WALK_RUN_LEVELS), asked of the library; no GPU needed"""
    a, b = C.c_int32(0), C.c_int32(0)
    check(load().csx_hqr_window(C.byref(a), C.byref(b)), "csx_hqr_window")
    return a.value, b.value


def level_schedule(level_ptr, waves, run_levels, work=None, run_work=0):
    """the launches [(wide, first level, end level)] of the level walk of ldlsol / schur / slusol / hqrsol_factor over the levels
    level_ptr (csx_level_schedule; csx_levelwalk.h); work: a figure per level, or none; no GPU needed"""
    lp = i32(level_ptr)
    nlev = len(lp) - 1
    out, count = np.zeros(3 * max(nlev, 1), np.int32), C.c_int32(0)
    w = None if work is None else np.ascontiguousarray(work, np.int64)
    check(load().csx_level_schedule(nlev, pi(lp), waves, run_levels, None if w is None else w.ctypes.data_as(C.POINTER(C.c_int64)),
                                    run_work, pi(out), C.byref(count)), "csx_level_schedule")
    return [(bool(out[3 * t]), int(out[3 * t + 1]), int(out[3 * t + 2])) for t in range(count.value)]


def row_view(p, i, descending=False):
    """(rp, rc, rpos): the rows of the square CSC pattern (p, i) with the column and the storage position of every entry, ordered by
    (column, position) ascending or both descending (csx_row_view; csx_levelwalk.h); no GPU needed"""
    p, i = i32(p), i32(i)
    n = len(p) - 1
    rp, rc, rpos = np.zeros(n + 1, np.int32), np.zeros(len(i), np.int32), np.zeros(len(i), np.int32)
    check(load().csx_row_view(n, pi(p), pi(i), int(descending), pi(rp), pi(rc), pi(rpos)), "csx_row_view")
    return rp, rc, rpos


SN_GEOMETRY_PLAN = ("chunk", "has_relaxed", "matrix_cores", "leaf_subtrees", "leaf_cols", "leaf_tasks", "leaf_slots",
                    "fundamental", "relaxed")
SN_GEOMETRY_DIR = ("steps", "tasks", "max_step_tasks", "cut_lines", "slots", "narrow", "medium", "wide", "one_triangle_steps")
SN_LAUNCHES = ("outside_wg", "outside", "thin1", "thin2", "thin4", "thin8", "thin16", "thin32", "combine", "mfma_w128",
               "mfma_leaf_ct1", "mfma_leaf_ct4", "mfma_ct1", "mfma_ct4", "tri16", "tri32", "tri64", "leaf", "use0")


def _sn_fields(fn, plan, what):
    n = C.c_int32(0)
    check(fn(plan, None, 0, C.byref(n)), what)
    out = (C.c_int64 * n.value)()
    check(fn(plan, out, n.value, C.byref(n)), what)
    return list(out)


def cholsol_sn_geometry(plan):
    """csx_cholsol_sn_geometry as a dict: the plan-wide fields, then "fwd" and "bwd" (include/csx.h has the order)"""
    v = _sn_fields(lib().csx_cholsol_sn_geometry, plan, "csx_cholsol_sn_geometry")
    a, b = len(SN_GEOMETRY_PLAN), len(SN_GEOMETRY_DIR)
    assert len(v) == a + 2 * b
    g = dict(zip(SN_GEOMETRY_PLAN, v[:a]))
    g["fwd"] = dict(zip(SN_GEOMETRY_DIR, v[a:a + b]))
    g["bwd"] = dict(zip(SN_GEOMETRY_DIR, v[a + b:]))
    return g


def cholsol_sn_launches(plan):
    """csx_cholsol_sn_launches as {"fwd": {kernel: launches}, "bwd": {...}}: what the plan's last solve enqueued"""
    v = _sn_fields(lib().csx_cholsol_sn_launches, plan, "csx_cholsol_sn_launches")
    k = len(SN_LAUNCHES)
    assert len(v) == 2 * k
    return {"fwd": dict(zip(SN_LAUNCHES, v[:k])), "bwd": dict(zip(SN_LAUNCHES, v[k:]))}


TRI_LIMITS = ("NARROW", "CHB", "CH_SUF", "TRW_MIN_ROW", "TRW_MAX_RHS", "TR64_MIN_RHS", "TR64_RUN", "TR64_RUN_MIN", "TC_MAX_N",
              "TC_THREADS", "COMP_MIN_COUNT", "COMP_MAX_ROWS", "PUSH_MAX_RHS", "FEW_MAX_RHS", "FEW_CPW", "COMP_LDS_MAX", "FEW_TILE_LDS",
              "WINDOW_LDS_MAX", "COLUMNS_LDS_MAX", "CHAIN_LINKS_NUM", "CHAIN_LINKS_DEN", "CHAIN_LEVELS_NUM", "WCOL_WIDE_ENTRIES",
              "WCHAIN_WIDE_ENTRIES", "WINDOW_SLACK", "STRIP_SHORT_COLS", "TL_WAVES_MAX", "LV_MAX_ROUNDS", "LV_DEVICE_MIN_TERMS",
              "LAUNCH_COUNTERS")
TRI_ROUTES = ("Ragged", "CompPush", "FewLds", "Few", "Local", "WColumns", "WColChain", "Columns", "ColChain", "Sequential", "Levels")
TRI_ROUTE_INFO = ("route", "lds", "grid", "G", "waves", "tile_rows", "chunks", "window", "threads", "rounds", "mate",
                  "band", "links", "col_state", "levels", "sequential", "chain_ok", "ncomp", "comp_max", "push_terms", "few_cpw",
                  "few_rows", "few_terms", "guard", "schedule", "comps_found", "comp_rows_found", "kind", "n", "terms")
TRI_LAUNCHES = ("level", "levels_one_wg", "chain", "sequential", "local_fwd", "local_bwd", "few_fwd", "few_bwd", "few_lds_fwd",
                "few_lds_bwd", "push_fwd", "push_bwd", "ragged", "columns_l", "columns_u", "colchain_lt", "colchain_ut",
                "wcolumns_256", "wcolumns_1024", "wcolchain_lt_2", "wcolchain_lt_12", "wcolchain_ut_2", "wcolchain_ut_12",
                "level_rows", "run_prefix_rows", "levels_rows_one_wg", "level_rows64", "run_prefix64", "levels_rows64_one_wg",
                "level_of")


def tri_limits():
    """the constants the triangular solve's routes are cut by (csx_trisolve.hip), asked of the library; no GPU needed: a dict by
    the names of TRI_LIMITS (include/csx.h: csx_tri_limits)"""
    out = (C.c_int32 * 32)()
    check(load().csx_tri_limits(out), "csx_tri_limits")
    return {name: int(out[k]) for k, name in enumerate(TRI_LIMITS)}


def tri_route_info(plan, nrhs, cholsol=None):
    """csx_tri_route_info as a dict by TRI_ROUTE_INFO, "route" as its name in TRI_ROUTES: what a solve of nrhs right-hand sides
    on this plan would run and what decided it; cholsol = 0 / 1: plan is a cholsol plan, asked about its forward / backward
    triangular plan (csx_cholsol_tri_route_info)"""
    if cholsol is None:
        v = _sn_fields(lambda h, out, cap, n: lib().csx_tri_route_info(h, nrhs, out, cap, n), plan, "csx_tri_route_info")
    else:
        v = _sn_fields(lambda h, out, cap, n: lib().csx_cholsol_tri_route_info(h, cholsol, nrhs, out, cap, n), plan,
                       "csx_cholsol_tri_route_info")
    assert len(v) == len(TRI_ROUTE_INFO)
    d = dict(zip(TRI_ROUTE_INFO, v))
    d["route"] = TRI_ROUTES[d["route"]]
    return d


def tri_launches(plan, cholsol=None):
    """csx_tri_launches as {kernel instance: launches} by TRI_LAUNCHES, the instances the plan's last solve did not enqueue left
    out; cholsol = 0 / 1: of the forward / backward triangular plan of a cholsol plan (csx_cholsol_tri_launches)"""
    if cholsol is None:
        v = _sn_fields(lib().csx_tri_launches, plan, "csx_tri_launches")
    else:
        v = _sn_fields(lambda h, out, cap, n: lib().csx_cholsol_tri_launches(h, cholsol, out, cap, n), plan,
                       "csx_cholsol_tri_launches")
    assert len(v) == len(TRI_LAUNCHES)
    return {k: c for k, c in zip(TRI_LAUNCHES, v) if c}


PRIM_LIMITS = ("SCAN_TILE", "SM_TILE", "RS_TILE", "RS_BINS", "RS_DESC_STARTS", "RS_SEGS", "RS_CHUNK_MIN", "RS_CHUNK_DIV",
               "EXPAND_GRID_MAX")
SORT_INSTANCES = ("none", "keys", "a", "v", "av_flat_flat", "av_flat_packed", "av_packed_packed", "av_packed_flat", "short_first",
                  "short_middle", "short_last")
SORT_INFO = ("bits", "passes", "widths", "nblocks", "chunk", "nchunks", "packed", "k16", "key_misalign", "instances", "count")


def prim_limits():
    """the constants the integer primitives are cut by (csx_sort.hip), asked of the library; no GPU needed: a dict by the names
    of PRIM_LIMITS (include/csx.h: csx_prim_limits)"""
    out = (C.c_int32 * len(PRIM_LIMITS))()
    check(load().csx_prim_limits(out), "csx_prim_limits")
    return {name: int(out[k]) for k, name in enumerate(PRIM_LIMITS)}


SPGEMM_LIMITS = ("SG_SEG", "SG_THREADS", "SG_DENSE_MAX", "SG_GLOBAL_WGS", "SG_HASH_MAXP", "HASH_LIMIT0", "HASH_LIMIT1", "HASH_LIMIT2",
                 "HASH_LIMIT3", "HASH_LIMIT4", "HASH_LIMIT5", "HASH_LIMIT6", "HASH_LIMIT7", "H2_MAXSEG", "H2_MAXLEN", "H2_MAXP",
                 "H1_SEG", "H1_MAXP", "H1_UN", "SGO_MAX", "SGO_SLOTS0", "SGO_CNT0", "SGO_SLOTS1", "SGO_CNT1", "SGO_SLOTS2", "SGO_CNT2",
                 "SGO_DENSE_WAVES", "SG_GRID_PER_CU", "INFO_FIELDS", "SGO_WAVES0", "SGO_WAVES1", "SGO_WAVES2", "SG_UN",
                 "SG_MIN_SLOTS", "SG_LDS_BUDGET", "SG_WGS_PER_CU_MAX", "SG_HASH_BINS", "SG_NARROW_BINS", "LAUNCH_SITES")
SPGEMM_SITES = (("products",) + tuple("spgemm_%s_%s" % (r, k) for r in ("symbolic", "values", "pattern")
                                      for k in ("dense", "hash", "global"))
                + tuple("hash1_%s_%d" % (v, b) for v in ("pattern", "values") for b in range(8))
                + tuple("hash2_%s_%d" % (v, b) for v in ("pattern", "values") for b in range(6))
                + ("compact", "dup_cols", "ordered2_0", "ordered2_1", "ordered2_2", "ordered_dense"))


def spgemm_limits():
    """the constants cs_multiply's bins, tables and staging are cut by (csx_spgemm.hip), asked of the library; no GPU needed: a
    dict by the names of SPGEMM_LIMITS (include/csx.h: csx_spgemm_limits)"""
    out = (C.c_int32 * 40)()
    check(load().csx_spgemm_limits(out), "csx_spgemm_limits")
    return {name: int(out[k]) for k, name in enumerate(SPGEMM_LIMITS)}


def spgemm_info():
    """what the last product on the device decided and launched (csx_spgemm_info; host state only): a dict with "bins" (32
    counts), "one_pass", "global_wgs", "cus", "ordered", "classes" (4 flags), "launches" and "grids" ({site of SPGEMM_SITES: n},
    the sites that were not launched left out)"""
    n = C.c_int32(0)
    out = (C.c_int64 * 256)()
    check(load().csx_spgemm_info(out, 256, C.byref(n)), "csx_spgemm_info")
    v, k = [int(x) for x in out[:n.value]], len(SPGEMM_SITES)
    assert n.value == 40 + 2 * k
    cnt, grid = v[40:40 + k], v[40 + k:]
    return {"bins": tuple(v[:32]), "one_pass": v[32], "global_wgs": v[33], "cus": v[34], "ordered": v[35], "classes": tuple(v[36:40]),
            "launches": {s: c for s, c in zip(SPGEMM_SITES, cnt) if c},
            "grids": {s: g for s, c, g in zip(SPGEMM_SITES, cnt, grid) if c}}


GMRES_LIMITS = ("GS_CHUNK", "GS_FAN", "GS_GROUP", "GS_TILE")
GS_PROJECT, GS_UPDATE, GS_SCALE, GS_COMBINE = 0, 1, 2, 3


def gmres_limits():
    """the constants of the ordered sum and of the Gram-Schmidt kernels of gmres() (csx_gmres.hip), asked of the library; no GPU
    needed: a dict by the names of GMRES_LIMITS (include/csx.h: csx_gmres_limits)"""
    out = (C.c_int32 * len(GMRES_LIMITS))()
    check(load().csx_gmres_limits(out), "csx_gmres_limits")
    return {name: int(out[k]) for k, name in enumerate(GMRES_LIMITS)}


def gs_work_len(rows, nrhs, nblocks):
    """doubles of the work vector the csx_gs_* calls need for blocks of rows x nrhs and a basis of nblocks; no GPU needed"""
    out = C.c_int64(0)
    check(load().csx_gs_work_len(rows, nrhs, nblocks, C.byref(out)), "csx_gs_work_len")
    return out.value


def gs_host(op, V, W, mask, coef=None, length=None, negate=False, nv=None):
    """csx_gs_host on numpy arrays: V (blocks, rows, nrhs), W (rows, nrhs) or None (combine), mask (nrhs).  GS_PROJECT -> h
    (nv, nrhs); GS_UPDATE -> (new W, nrm2); GS_SCALE (nv: the slot) -> new V; GS_COMBINE -> U.  The inputs are left as they
    are; where a column is masked, the outputs hold what the inputs held (h, nrm2: NaN; U: NaN).  No GPU needed."""
    V = np.array(V, dtype=np.float64)
    nb, rows, k = V.shape
    nv = nb if nv is None else nv
    W = None if W is None else np.array(W, dtype=np.float64).reshape(rows, k)
    m = i32(mask)
    cf = None if coef is None else f64(coef)
    ln = None if length is None else i32(length)
    out = {GS_PROJECT: np.full((nv, k), np.nan), GS_UPDATE: np.full(k, np.nan), GS_SCALE: None,
           GS_COMBINE: np.full((rows, k), np.nan)}[op]
    check(load().csx_gs_host(op, rows, k, nv, pd(V), pd(W), pi(m), 1 if negate else 0, pd(cf), pi(ln), pd(out)), "csx_gs_host")
    return {GS_PROJECT: out, GS_UPDATE: (W, out), GS_SCALE: V, GS_COMBINE: out}[op]


PATTERN_OUTER_LIMITS = ("PO_LANES", "PO_CHUNK", "PO_WAVE_CHUNK", "PO_FLIGHT", "PO_KEPT")


def pattern_outer_limits():
    """the constants of csx_pattern_outer's value rule and kernel (csx_pattern_outer.h), asked of the library; no GPU needed: a
    dict by the names of PATTERN_OUTER_LIMITS (include/csx.h: csx_pattern_outer_limits)"""
    out = (C.c_int64 * len(PATTERN_OUTER_LIMITS))()
    check(load().csx_pattern_outer_limits(out), "csx_pattern_outer_limits")
    return {name: int(out[k]) for k, name in enumerate(PATTERN_OUTER_LIMITS)}


def pattern_outer_host(m, n, p, i, U, V, nrhs, alpha=1.0, sym=False):
    """csx_pattern_outer_host on numpy arrays: the nnz values of alpha U V' on the pattern (p, i); U m x nrhs, V n x nrhs.  No GPU
    needed."""
    p, i = i32(p), i32(i)
    U, V = f64(np.asarray(U, dtype=np.float64).reshape(-1)), f64(np.asarray(V, dtype=np.float64).reshape(-1))
    out = np.full(max(int(p[n]), 1), np.nan)
    check(load().csx_pattern_outer_host(m, n, pi(p), pi(i), nrhs, 1 if sym else 0, float(alpha), pd(U), pd(V), pd(out)),
          "csx_pattern_outer_host")
    return out[:int(p[n])]


def assemble_pullback_host(sp, src, g):
    """csx_assemble_pullback_host on numpy arrays: the nz triplet gradients of the slot gradients g through a plan's sp, src
    (csx_assemble_plan_host).  No GPU needed."""
    sp, src, g = i32(sp), i32(src), f64(g)
    nnz, nz = len(sp) - 1, len(src)
    out = np.full(max(nz, 1), np.nan)
    check(load().csx_assemble_pullback_host(nnz, nz, pi(sp), pi(src), pd(g), pd(out)), "csx_assemble_pullback_host")
    return out[:nz]


BGS_LIMITS = ("GS_CHUNK", "GS_FAN", "BGS_MAXW", "BGS_GROUP", "BGS_TILE")
BGS_GRAM, BGS_UPDATE, BGS_COMBINE = 0, 1, 2


def bgs_limits():
    """the constants of the ordered sum and of the block kernels of eigsh() (csx_bgs.hip), asked of the library; no GPU needed:
    a dict by the names of BGS_LIMITS (include/csx.h: csx_bgs_limits)"""
    out = (C.c_int32 * len(BGS_LIMITS))()
    check(load().csx_bgs_limits(out), "csx_bgs_limits")
    return {name: int(out[k]) for k, name in enumerate(BGS_LIMITS)}


def bgs_work_len(rows, b, q, nblocks):
    """doubles of the work vector the csx_bgs_* calls need for rows x b basis blocks (nblocks at most) and a rows x q block;
    no GPU needed"""
    out = C.c_int64(0)
    check(load().csx_bgs_work_len(rows, b, q, nblocks, C.byref(out)), "csx_bgs_work_len")
    return out.value


def bgs_host(op, V, W=None, coef=None, negate=False, q=None):
    """csx_bgs_host on numpy arrays: V (blocks, rows, b), W (rows, q) or None (combine: q from coef (blocks, b, q), or given).
    BGS_GRAM -> sums (blocks, b, q); BGS_UPDATE -> the new W; BGS_COMBINE -> U.  The inputs are left as they are.  No GPU needed."""
    V = np.array(V, dtype=np.float64)
    nv, rows, b = V.shape
    W = None if W is None else np.array(W, dtype=np.float64)
    W = W[:, None] if W is not None and W.ndim == 1 else W
    cf = None if coef is None else f64(coef)
    q = W.shape[1] if W is not None else (int(q) if q is not None else cf.shape[-1])
    out = {BGS_GRAM: np.full((nv, b, q), np.nan), BGS_UPDATE: None, BGS_COMBINE: np.full((rows, q), np.nan)}[op]
    check(load().csx_bgs_host(op, rows, b, q, nv, pd(V), pd(W), 1 if negate else 0, pd(cf), pd(out)), "csx_bgs_host")
    return W if op == BGS_UPDATE else out


def _u32(a):
    return None if a is None else np.array(a, dtype=np.uint32)     # (a copy: the library writes its inputs back)


def _vptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def prim_scan(values, in_place=False):
    """scan_exclusive_i32 of a host array (csx_prim_scan): (out[0 .. n], total, the input as the device left it -- None in place)"""
    a = np.array(values, dtype=np.int32)
    out, total = np.full(len(a) + 1, -1, np.int32), C.c_int64(-1)
    check(lib().csx_prim_scan(pi(a), pi(out), len(a), 1 if in_place else 0, C.byref(total)), "csx_prim_scan")
    return out, total.value, (None if in_place else a)


def prim_suffix_min(values):
    """suffix_min_i32 of a host array (csx_prim_suffix_min)"""
    p = np.array(values, dtype=np.int32)
    check(lib().csx_prim_suffix_min(pi(p), len(p)), "csx_prim_suffix_min")
    return p


def prim_expand_columns(Ap, fill=-1):
    """expand_columns under the column pointers Ap (csx_prim_expand_columns): (col, Ap as the device left it)"""
    p = np.array(Ap, dtype=np.int32)
    col = np.full(int(p[-1]), fill, np.int32)
    check(lib().csx_prim_expand_columns(pi(p), len(p) - 1, len(col), pi(col)), "csx_prim_expand_columns")
    return col, p


def prim_boundaries(sorted_key, nkeys, misalign_words=0, fill=-1):
    """boundaries_from_sorted (csx_prim_boundaries): (ptr[0 .. nkeys], the keys as the device left them)"""
    k = _u32(sorted_key)
    ptr = np.full(nkeys + 1, fill, np.int32)
    check(lib().csx_prim_boundaries(_vptr(k), len(k), nkeys, pi(ptr), misalign_words), "csx_prim_boundaries")
    return ptr, k


def prim_sort(key, a=None, v=None, key_limit=0xFFFFFFFF, want_key=True, expand_ptr=None, nkeys=None, misalign_words=0):
    """stable_sort_by_key_ex on host arrays (csx_prim_sort).  a (uint32), v (float64), expand_ptr (column pointers over the
    records) optional; want_key: ask for the sorted keys; nkeys not None: ask for the pointer array of nkeys keys.  A dict:
    out_key, out_a, out_v, out_ptr (None where not asked for), and key, a, v, expand_ptr as the device left the inputs."""
    k, aa = _u32(key), _u32(a)
    vv = None if v is None else np.array(v, dtype=np.float64)
    xp = None if expand_ptr is None else np.array(expand_ptr, dtype=np.int32)
    n = len(k)
    ok = np.full(n, 0xDEADBEEF, np.uint32) if want_key else None
    oa = np.full(n, 0xDEADBEEF, np.uint32) if (aa is not None or xp is not None) else None
    ov = np.full(n, -777.0, np.float64) if vv is not None else None
    op = np.full(nkeys + 1, -1, np.int32) if nkeys is not None else None
    check(lib().csx_prim_sort(_vptr(k), _vptr(aa), pd(vv), n, key_limit, _vptr(ok), _vptr(oa), pd(ov), pi(xp),
                              0 if xp is None else len(xp) - 1, pi(op), 0 if nkeys is None else nkeys, misalign_words),
          "csx_prim_sort")
    return {"out_key": ok, "out_a": oa, "out_v": ov, "out_ptr": op, "key": k, "a": aa, "v": vv, "expand_ptr": xp}


def prim_sort_info():
    """what the last sort of this process decided (csx_prim_sort_info; host state only): a dict by SORT_INFO, "widths" and
    "instances" (names of SORT_INSTANCES) one per pass"""
    out = (C.c_int64 * 17)()
    check(load().csx_prim_sort_info(out, 17), "csx_prim_sort_info")
    v = [int(x) for x in out]
    passes = v[1]
    return {"bits": v[0], "passes": passes, "widths": tuple(v[2:2 + passes]), "nblocks": v[6], "chunk": v[7], "nchunks": v[8],
            "packed": v[9], "k16": v[10], "key_misalign": v[11], "instances": tuple(SORT_INSTANCES[i] for i in v[12:12 + passes]),
            "count": v[16]}


BLOCK_LIMITS = ("LU_MAX_M", "LU_MIN_COMPONENTS", "QR_MAX_M", "QR_MIN_COMPONENTS", "HAPPLY_MAX_LEVELS")


def block_limits():
    """the cuts of csx_lu_blocks, csx_qr_blocks and csx_happly, asked of the library; no GPU needed: a dict by the names of
    BLOCK_LIMITS (include/csx.h: csx_block_limits)"""
    out = (C.c_int32 * len(BLOCK_LIMITS))()
    check(load().csx_block_limits(out), "csx_block_limits")
    return {name: int(out[k]) for k, name in enumerate(BLOCK_LIMITS)}


BTF_LIMITS = ("BTF_SMALL", "RF_MAX", "RF_WAVES", "RHS_TILE", "TERM_CHUNK", "TERM_GROUP")


def btf_limits():
    """the cuts and strides of btf_factor's solve kernel and of the refactor kernel, asked of the library; no GPU needed: a dict
    by the names of BTF_LIMITS (include/csx.h: csx_btf_limits)"""
    out = (C.c_int32 * len(BTF_LIMITS))()
    check(load().csx_btf_limits(out), "csx_btf_limits")
    return {name: int(out[k]) for k, name in enumerate(BTF_LIMITS)}


def prim_components(n, p, i, skip_first=0, skip_last=0, order=0):
    """connected_components + group_by_root on host arrays (csx_prim_components).  A dict: root, nodes, first, count (ncomp
    entries each), comp_of_pos, ncomp, maxc, malformed, and p, i as the device left them.  With malformed set the other
    results are None."""
    pp, ii = np.array(p, dtype=np.int32), np.array(i, dtype=np.int32)
    root, nodes, cop = np.full(n, -7, np.int32), np.full(n, 0xDEADBEEF, np.uint32), np.full(n, -7, np.int32)
    first, count = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    ncomp, maxc, bad = C.c_int32(-1), C.c_int32(-1), C.c_int(-1)
    check(lib().csx_prim_components(n, pi(pp), pi(ii), skip_first, skip_last, order, pi(root), _vptr(nodes), pi(first), pi(count),
                                    pi(cop), C.byref(ncomp), C.byref(maxc), C.byref(bad)), "csx_prim_components")
    out = {"ncomp": ncomp.value, "maxc": maxc.value, "malformed": bad.value, "p": pp, "i": ii,
           "root": None, "nodes": None, "first": None, "count": None, "comp_of_pos": None}
    if not bad.value:
        out.update(root=root, nodes=nodes, first=first[:ncomp.value], count=count[:ncomp.value], comp_of_pos=cop)
    return out


def exported_symbols():
    return sorted(list(_PROTOS) + ["csx_last_error", "csx_host_free"])


def check(status, what=""):
    if status == OK:
        return
    if status == EZEROPIVOT:
        raise ZeroDivisionError("float division by zero")
    if status == ENOTSPD:
        raise NotPositiveDefinite(what or "matrix is not positive definite")
    if status == EINVAL:
        raise ValueError("libcsx: bad argument" + (" in " + what if what else ""))
    raise CsxError("libcsx %s: %s" % (what, load().csx_last_error().decode("utf-8", "replace")))


def init(device=None):
    """Bind this process to one GPU (LOCAL_RANK by default) and create the context."""
    global _ready
    lib = load()
    if not _ready:
        if device is None:
            device = int(os.environ.get("CSX_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        st = lib.csx_init(int(device))
        if st != OK:
            raise CsxError("csx_init(%d) failed: %s -- the MI355X path has no CPU fallback"
                           % (device, lib.csx_last_error().decode("utf-8", "replace")))
        _ready = True
    return lib


def lib():
    return init()


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pi(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def pd(a):
    return None if a is None else a.ctypes.data_as(_f64p)


def new_handle():
    return H(0)


def free(h):
    if h and _lib is not None and _ready:
        _lib.csx_free(h)


def sync():
    check(lib().csx_sync(), "csx_sync")


def device_info():
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    mem = C.c_int64(0)
    check(lib().csx_device_info(name, 256, C.byref(cus), C.byref(mem)), "csx_device_info")
    return name.value.decode(), cus.value, mem.value


class option(object):
    """with _csx.option("spgemm.one_pass", 0): ...   -- a kernel-selection override for tests (csx_set_option)"""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), int(value)

    def __enter__(self):
        old = C.c_int(0)
        check(lib().csx_get_option(self.name, C.byref(old)), "csx_get_option")
        self.old = old.value                      # the value in force on entry: nested blocks restore correctly
        check(lib().csx_set_option(self.name, self.value), "csx_set_option")
        return self

    def __exit__(self, *exc):
        check(lib().csx_set_option(self.name, self.old), "csx_set_option")
        return False


class Timer(object):
    """HIP-event timer on the library's stream (the stream the kernels run on)."""

    def __enter__(self):
        check(lib().csx_timer_start(), "csx_timer_start")
        self.ms = None
        return self

    def __exit__(self, *exc):
        ms = C.c_double(0.0)
        check(lib().csx_timer_stop(C.byref(ms)), "csx_timer_stop")
        self.ms = ms.value
        return False
