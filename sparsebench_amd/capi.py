"""ctypes binding of the C-ABI HIP layer (include/sbhip.h -> lib/libsbhip.so).

This is plumbing only: every call goes straight into the shared library.  There is
no CPU fallback -- if the library is missing, or no MI355X is visible, using the
hot path raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBHIP_LIBRARY") or os.path.join(HERE, "lib", "libsbhip.so")  # override: an instrumented copy

# every symbol include/sbhip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "sb_init", "sb_finalize", "sb_is_initialized", "sb_device_count", "sb_device_name",
    "sb_num_cus", "sb_sync", "sb_stream", "sb_malloc", "sb_free", "sb_memset", "sb_h2d",
    "sb_d2h", "sb_d2d", "sb_is_device_ptr", "sb_event_create", "sb_event_record",
    "sb_event_elapsed_ms", "sb_event_destroy", "sb_crs_upload", "sb_scs_upload",
    "sb_matrix_free", "sb_matrix_nr", "sb_matrix_nc", "sb_matrix_is_permuted",
    "sb_matrix_spmv_bytes", "sb_spmv", "sb_spmv_native", "sb_permute", "sb_unpermute",
    "sb_waxpby", "sb_ddot_async", "sb_ddot", "sb_ddot_partials", "sb_reduce_final",
    "sb_comm_unique_id", "sb_comm_init", "sb_comm_finalize", "sb_comm_rank", "sb_comm_size",
    "sb_comm_reduction", "sb_halo_create", "sb_halo_free", "sb_halo_exchange", "sb_cg_create",
    "sb_cg_free", "sb_cg_set_fused", "sb_cg_set_graph", "sb_cg_solve", "sb_cg_run_iters",
    "sb_cg_history", "sb_cg_solution", "sb_cg_check_residual", "sb_cg_region_ms", "sb_version",
    "sb_comm_allgather_bytes", "sb_comm_alltoallv_ints", "sb_comm_barrier", "sb_cg_loop_ms",
    "sb_cg_spmv_timing", "sb_cg_spmv_ms", "sb_cg_spmv_us_series", "sb_cg_counters", "sb_debug_stream_read_gbs",
    "sb_matrix_pack_level", "sb_set_external_ids", "sb_spmv_native_dot", "sb_matrix_use_packed", "sb_matrix_stream_bytes",
    "sb_matrix_packed_mode", "sb_matrix_crs_kernel", "sb_matrix_lds_window", "sb_matrix_pattern_classes", "sb_matrix_row_patterns", "sb_matrix_row_programs", "sb_comm_p2p_handle", "sb_comm_p2p_open", "sb_comm_p2p_enabled", "sb_halo_p2p_enabled", "sb_cg_start", "sb_cg_finish", "sb_cg_vector_phase", "sb_cg_launches_per_body",
    "sb_comm_init_transport", "sb_comm_p2p_reason", "sb_halo_p2p_reason",
    "sb_comm_data_plane", "sb_comm_data_plane_selected", "sb_comm_rccl_info", "sb_cg_phase_timing", "sb_cg_phase_ms",
    "sb_comm_halo_push_inside", "sb_comm_halo_fold", "sb_comm_halo_fold_selected", "sb_cg_halo_fold", "sb_lab_build", "sb_cg_collectives_per_body",
    "sb_cg_set_fuse_p", "sb_cg_fuse_p", "sb_cg_set_fuse_alpha", "sb_cg_set_fuse_beta",
    "sb_cg_update_p_native", "sb_cg_update_r_native", "sb_cg_scalar_native", "sb_cg_x_finalize_native", "sb_cg_dot_spans_native",
    "sb_waxpby_sdev_native", "sb_cg_update_p_launch", "sb_cg_update_r_launch",
    "sb_malloc_host_visible", "sb_host_visible_reason", "sb_malloc_pinned_host", "sb_free_pinned_host", "sb_copy_counters",
    "sb_region_begin", "sb_region_end", "sb_region_seconds", "sb_region_reset",
    "sb_is_pinned_host_ptr", "sb_mem_free_bytes",
    "sb_set_dot_order", "sb_dot_order", "sb_cg_set_dot_order", "sb_cg_dot_order",
    "sb_crs_upload_f32", "sb_scs_upload_f32", "sb_matrix_precision", "sb_spmv_f32", "sb_spmv_native_dot_f32", "sb_permute_f32",
    "sb_unpermute_f32", "sb_waxpby_f32", "sb_ddot_f32", "sb_ddot_partials_f32", "sb_reduce_final_f32", "sb_cg_create_f32",
    "sb_cg_solution_f32", "sb_comm_reduction_f32", "sb_rank_reduce_f32", "sb_halo_exchange_f32",
    "sb_set_sp_mirror", "sb_sp_mirror", "sb_matrix_all_row_programs",
    "sb_cg_update_p_native_f32", "sb_cg_update_r_native_f32", "sb_cg_scalar_native_f32", "sb_cg_x_finalize_native_f32",
    "sb_axpy_sdev_native_f32", "sb_dot_l1_native_f32", "sb_waxpby_stop_native_f32", "sb_cg_update_p_launch_f32",
    "sb_cg_update_r_launch_f32", "sb_dot_l1_launch_f32", "sb_stream_launch_f32",
    "sb_matrix_place","sb_matrix_place_at", "sb_matrix_place_home", "sb_placement_arena_bytes", "sb_placement_probe", "sb_matrix_place_fresh", "sb_matrix_place_commit", "sb_matrix_placement", "sb_matrix_placement_report", "sb_matrix_debug_ptrs", "sb_cg_debug_ptrs",
    "sb_gmres_create", "sb_gmres_free", "sb_gmres_set_fused", "sb_gmres_restart", "sb_gmres_launches_per_step", "sb_gmres_solve",
    "sb_gmres_start", "sb_gmres_run_steps", "sb_gmres_finish", "sb_gmres_history", "sb_gmres_solution", "sb_gmres_check_residual",
    "sb_gmres_loop_ms", "sb_gmres_counters", "sb_multidot", "sb_multiaxpy_sub", "sb_debug_sqrt_div",
    "sb_spmmv_native", "sb_spmmv_native_dot", "sb_block_interleave", "sb_block_deinterleave", "sb_matrix_spmmv_bytes",
    "sb_cgb_create", "sb_cgb_free", "sb_cgb_nrhs", "sb_cgb_launches_per_body", "sb_cgb_solve", "sb_cgb_start", "sb_cgb_run_iters",
    "sb_cgb_finish", "sb_cgb_iterations", "sb_cgb_history", "sb_cgb_solution", "sb_cgb_check_residual", "sb_cgb_loop_ms",
    "sb_cgb_counters", "sb_block_vec_native", "sb_block_vec_launch", "sb_cgb_update_p_native", "sb_cgb_x_finalize_native",
    "sb_cgb_rows_launch", "sb_gmres_group_launch",
    "sb_gmres_scale_launch", "sb_gmres_step_launch", "sb_gmres_multidot_native", "sb_gmres_finish_dots_native", "sb_gmres_project_native",
    "sb_gmres_multiadd_native", "sb_gmres_scale_native", "sb_gmres_rr_native", "sb_gmres_step_native", "sb_gmres_backsolve_native",
    "sb_matrix_diagonal", "sb_pcg_create", "sb_pcg_free", "sb_pcg_solve", "sb_pcg_start", "sb_pcg_run_iters", "sb_pcg_finish",
    "sb_pcg_history", "sb_pcg_solution", "sb_pcg_check_residual", "sb_pcg_dinv", "sb_pcg_launches_per_body", "sb_pcg_loop_ms",
    "sb_pcg_counters", "sb_pcg_update_r_native", "sb_pcg_update_r_launch", "sb_pcg_collectives_per_body", "sb_pcg_local_reduce_native",
    "sb_pcg_create_sgs", "sb_pcg_precond", "sb_pcg_colours", "sb_pcg_colouring", "sb_pcg_apply_precond", "sb_pcg_precond_bytes",
    "sb_pcg_apply_precond_ms",
    "sb_pcg_create_mg", "sb_pcg_levels", "sb_pcg_level_rows", "sb_pcg_level_colours",
    "sb_pcg_create_mg_p", "sb_pcg_mg_fw_probe",
    "sb_pcg_create_poly", "sb_pcg_poly_steps", "sb_pcg_poly_interval", "sb_pcg_poly_coeffs", "sb_pcg_poly_rowbound",
    "sb_pcg_poly_update_r_native", "sb_pcg_poly_step_native", "sb_pcg_poly_step_launch",
    "sb_pcg_create_mg_poly", "sb_pcg_mg_poly_level_steps", "sb_pcg_mg_poly_interval", "sb_pcg_mg_poly_coeffs", "sb_pcg_mg_poly_probe",
    "sb_pcg_mg_poly_first_native", "sb_pcg_mg_poly_first_launch",
    "sb_bicgstab_create", "sb_bicgstab_free", "sb_bicgstab_solve", "sb_bicgstab_start", "sb_bicgstab_run_iters", "sb_bicgstab_finish",
    "sb_bicgstab_history", "sb_bicgstab_solution", "sb_bicgstab_check_residual", "sb_bicgstab_dinv", "sb_bicgstab_launches_per_body",
    "sb_bicgstab_loop_ms", "sb_bicgstab_counters", "sb_bicgstab_update_p_native", "sb_bicgstab_update_s_native",
    "sb_bicgstab_dot2_native", "sb_bicgstab_update_xr_native", "sb_bicgstab_reduce_native", "sb_bicgstab_launch",
    "sb_bicgstab_create_pre", "sb_bicgstab_precond", "sb_bicgstab_plan_update_p_native", "sb_bicgstab_plan_update_s_native",
    "sb_matrix_resident_share", "sb_resident_share_rule",
    "sb_matrix_galerkin", "sb_csr_rows", "sb_csr_nnz", "sb_csr_copy", "sb_csr_stats", "sb_csr_free",
    "sb_matrix_aggregate", "sb_matrix_sa_prolongation",
    "sb_gmres_create_pre", "sb_gmres_create_dinv", "sb_gmres_precond", "sb_gmres_dinv", "sb_gmres_pre_scale_native", "sb_gmres_pre_multiupdate_native",
    "sb_gmres_pre_step_native",
]

_lib = None
vp = C.c_void_p
u32 = C.c_uint32


def load():
    """Load libsbhip.so (no device is touched until sb_init)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "sparsebench_amd: %s is missing -- build it with `make hip` (hipcc, gfx950). "
            "There is no CPU fallback for the hot path." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    sig = {
        "sb_init": (None, [C.c_int]),
        "sb_finalize": (None, []),
        "sb_is_initialized": (C.c_int, []),
        "sb_device_count": (C.c_int, []),
        "sb_device_name": (C.c_char_p, []),
        "sb_num_cus": (C.c_int, []),
        "sb_sync": (None, []),
        "sb_stream": (vp, []),
        "sb_malloc": (vp, [C.c_size_t]),
        "sb_free": (None, [vp]),
        "sb_memset": (None, [vp, C.c_int, C.c_size_t]),
        "sb_h2d": (None, [vp, vp, C.c_size_t]),
        "sb_d2h": (None, [vp, vp, C.c_size_t]),
        "sb_d2d": (None, [vp, vp, C.c_size_t]),
        "sb_is_device_ptr": (C.c_int, [vp]),
        "sb_event_create": (vp, []),
        "sb_event_record": (None, [vp]),
        "sb_event_elapsed_ms": (C.c_float, [vp, vp]),
        "sb_event_destroy": (None, [vp]),
        "sb_crs_upload": (vp, [u32, u32, vp, vp, vp]),
        "sb_scs_upload": (vp, [u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]),
        "sb_matrix_free": (None, [vp]),
        "sb_matrix_nr": (u32, [vp]),
        "sb_matrix_nc": (u32, [vp]),
        "sb_matrix_is_permuted": (C.c_int, [vp]),
        "sb_matrix_spmv_bytes": (C.c_double, [vp]),
        "sb_spmv": (None, [vp, vp, vp]),
        "sb_spmv_native": (None, [vp, vp, vp]),
        "sb_permute": (None, [vp, vp, vp]),
        "sb_unpermute": (None, [vp, vp, vp]),
        "sb_waxpby": (None, [u32, C.c_double, vp, C.c_double, vp, vp]),
        "sb_ddot_async": (None, [u32, vp, vp, vp]),
        "sb_ddot": (C.c_double, [u32, vp, vp]),
        "sb_ddot_partials": (None, [u32, vp, vp, vp]),
        "sb_reduce_final": (None, [u32, vp, vp]),
        "sb_comm_unique_id": (None, [vp]),
        "sb_comm_init": (None, [C.c_int, C.c_int, vp]),
        "sb_comm_finalize": (None, []),
        "sb_comm_rank": (C.c_int, []),
        "sb_comm_size": (C.c_int, []),
        "sb_comm_reduction": (None, [vp, C.c_int]),
        "sb_halo_create": (vp, [u32, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                C.c_int, vp]),
        "sb_halo_free": (None, [vp]),
        "sb_halo_exchange": (None, [vp, vp]),
        "sb_cg_create": (vp, [vp, vp, vp, vp]),
        "sb_cg_free": (None, [vp]),
        "sb_cg_set_fused": (None, [vp, C.c_int]),
        "sb_cg_set_graph": (None, [vp, C.c_int]),
        "sb_cg_solve": (C.c_int, [vp, C.c_int, C.c_double]),
        "sb_cg_run_iters": (None, [vp, C.c_int]),
        "sb_cg_history": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "sb_cg_solution": (None, [vp, vp]),
        "sb_cg_check_residual": (C.c_double, [vp]),
        "sb_cg_region_ms": (None, [vp, vp]),
        "sb_version": (C.c_char_p, []),
        "sb_comm_allgather_bytes": (None, [vp, C.c_int, vp]),
        "sb_comm_alltoallv_ints": (None, [vp, vp, vp, vp, vp, vp]),
        "sb_comm_barrier": (None, []),
        "sb_cg_loop_ms": (C.c_double, [vp]),
        "sb_cg_spmv_timing": (None, [vp, C.c_int]),
        "sb_cg_spmv_ms": (C.c_double, [vp, C.POINTER(C.c_int)]),
        "sb_cg_spmv_us_series": (C.c_int, [vp, C.POINTER(C.c_float), C.c_int]),
        "sb_cg_counters": (None, [vp, vp]),
        # the CG loop's kernels alone (blocking test entries) and the launches of its two streaming kernels
        "sb_cg_update_p_native": (C.c_int, [C.c_int, u32, vp, vp, vp, C.c_int, u32, vp, vp, vp, vp]),
        "sb_cg_update_r_native": (C.c_int, [C.c_int, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "sb_cg_scalar_native": (C.c_int, [C.c_int, C.c_int, u32, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
        "sb_cg_x_finalize_native": (C.c_int, [u32, vp, vp, vp, vp, vp]),
        "sb_cg_dot_spans_native": (C.c_int, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp]),
        "sb_waxpby_sdev_native": (C.c_int, [u32, vp, C.c_int, vp, vp, vp, vp]),
        "sb_cg_update_p_launch": (None, [u32, vp]),
        "sb_cg_update_r_launch": (None, [u32, C.c_int, vp]),
        "sb_debug_stream_read_gbs": (C.c_double, [C.c_size_t, C.c_int]),
        "sb_matrix_pack_level": (C.c_int, [vp]),
        "sb_matrix_use_packed": (None, [vp, C.c_int]),
        "sb_matrix_resident_share": (C.c_int, [vp, C.c_int]),
        "sb_resident_share_rule": (C.c_int, [C.c_double, C.c_uint32, C.c_int]),
        "sb_set_external_ids": (None, [vp, C.c_uint32]),
        "sb_spmv_native_dot": (C.c_int, [vp, vp, vp, vp]),
        "sb_matrix_stream_bytes": (C.c_double, [vp]),
        "sb_matrix_packed_mode": (C.c_int, [vp]),
        "sb_matrix_crs_kernel": (C.c_int, [vp]),
        "sb_matrix_lds_window": (C.c_uint32, [vp]),
        "sb_matrix_pattern_classes": (C.c_uint32, [vp]),
        "sb_matrix_row_patterns": (C.c_uint32, [vp, C.POINTER(C.c_uint32)]),
        "sb_matrix_row_programs": (C.c_uint32, [vp, C.POINTER(C.c_uint32)]),
        "sb_cg_vector_phase": (C.c_int, [vp]),
        "sb_cg_launches_per_body": (C.c_int, [vp]),
        "sb_cg_start": (None, [vp, C.c_int, C.c_double]),
        "sb_cg_finish": (C.c_int, [vp]),
        "sb_comm_init_transport": (None, [C.c_int, C.c_int, vp]),
        "sb_comm_p2p_handle": (C.c_int, [vp]),
        "sb_comm_p2p_open": (C.c_int, [vp]),
        "sb_comm_p2p_enabled": (C.c_int, []),
        "sb_halo_p2p_enabled": (C.c_int, [vp]),
        "sb_comm_p2p_reason": (C.c_char_p, []),
        "sb_halo_p2p_reason": (C.c_char_p, [vp]),
        "sb_comm_data_plane": (None, [C.c_int]),
        "sb_comm_data_plane_selected": (C.c_int, []),
        "sb_comm_halo_push_inside": (None, [C.c_int]),
        "sb_comm_halo_fold": (None, [C.c_int]),
        "sb_comm_halo_fold_selected": (C.c_int, []),
        "sb_cg_halo_fold": (C.c_int, [vp]),
        "sb_lab_build": (C.c_int, []),
        "sb_cg_collectives_per_body": (C.c_int, [vp]),
        "sb_cg_set_fuse_p": (None, [vp, C.c_int]),
        "sb_cg_fuse_p": (C.c_int, [vp]),
        "sb_cg_set_fuse_alpha": (None, [vp, C.c_int]),
        "sb_cg_set_fuse_beta": (None, [vp, C.c_int]),
        "sb_comm_rccl_info": (C.c_int, [C.POINTER(C.c_int)]),
        "sb_cg_phase_timing": (None, [vp, C.c_int]),
        "sb_cg_phase_ms": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
        "sb_malloc_host_visible": (vp, [C.c_size_t]),
        "sb_host_visible_reason": (C.c_char_p, []),
        "sb_malloc_pinned_host": (vp, [C.c_size_t]),
        "sb_free_pinned_host": (None, [vp]),
        "sb_copy_counters": (None, [C.POINTER(C.c_uint64)]),
        "sb_region_begin": (None, [C.c_int]),
        "sb_region_end": (None, [C.c_int]),
        "sb_region_seconds": (C.c_double, [C.c_int, C.POINTER(C.c_uint64)]),
        "sb_region_reset": (None, []),
        "sb_is_pinned_host_ptr": (C.c_int, [vp]),
        "sb_mem_free_bytes": (C.c_size_t, []),
        "sb_matrix_place": (None, [vp, C.c_int, C.c_int]),
        "sb_matrix_place_commit": (None, [vp]),
        "sb_matrix_place_fresh": (None, [vp]),
        "sb_matrix_place_at": (None, [vp, vp, vp]),
        "sb_matrix_place_home": (None, [vp]),
        "sb_placement_arena_bytes": (C.c_size_t, [vp]),
        "sb_placement_probe": (C.c_float, [vp, vp]),
        "sb_matrix_placement": (None, [vp, C.POINTER(C.c_int)]),
        "sb_matrix_debug_ptrs": (None, [vp, C.POINTER(C.c_uint64)]),
        "sb_matrix_placement_report": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "sb_cg_debug_ptrs": (None, [vp, C.POINTER(C.c_uint64)]),
        "sb_set_dot_order": (None, [C.c_int]),
        "sb_dot_order": (C.c_int, []),
        "sb_cg_set_dot_order": (None, [vp, C.c_int]),
        "sb_cg_dot_order": (C.c_int, [vp]),
        # single precision
        "sb_crs_upload_f32": (vp, [u32, u32, vp, vp, vp]),
        "sb_scs_upload_f32": (vp, [u32, u32, u32, u32, u32, u32, vp, vp, vp, vp, vp, vp]),
        "sb_matrix_precision": (C.c_int, [vp]),
        "sb_spmv_f32": (None, [vp, vp, vp]),
        "sb_spmv_native_dot_f32": (C.c_int, [vp, vp, vp, vp]),
        "sb_permute_f32": (None, [vp, vp, vp]),
        "sb_unpermute_f32": (None, [vp, vp, vp]),
        "sb_waxpby_f32": (None, [u32, C.c_float, vp, C.c_float, vp, vp]),
        "sb_ddot_f32": (C.c_float, [u32, vp, vp]),
        "sb_ddot_partials_f32": (None, [u32, vp, vp, vp]),
        "sb_reduce_final_f32": (None, [u32, vp, vp]),
        "sb_cg_create_f32": (vp, [vp, vp, vp, vp]),
        "sb_cg_solution_f32": (None, [vp, vp]),
        "sb_comm_reduction_f32": (None, [vp, C.c_int]),
        "sb_rank_reduce_f32": (C.c_float, [vp, C.c_int, C.c_int]),
        "sb_halo_exchange_f32": (None, [vp, vp]),
        "sb_set_sp_mirror": (None, [C.c_int]),
        "sb_sp_mirror": (C.c_int, []),
        "sb_matrix_all_row_programs": (C.c_int, [vp]),
        "sb_cg_update_p_native_f32": (C.c_int, [C.c_int, u32, vp, vp, vp, C.c_int, u32, vp, vp, vp, vp, vp]),
        "sb_cg_update_r_native_f32": (C.c_int, [C.c_int, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]),
        "sb_cg_scalar_native_f32": (C.c_int, [C.c_int, C.c_int, u32, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "sb_cg_x_finalize_native_f32": (C.c_int, [u32, vp, vp, vp, vp, vp, vp]),
        "sb_axpy_sdev_native_f32": (C.c_int, [u32, vp, C.c_int, vp, vp, vp, vp, vp]),
        "sb_dot_l1_native_f32": (C.c_int, [u32, vp, vp, vp, C.c_int]),
        "sb_waxpby_stop_native_f32": (C.c_int, [u32, C.c_float, vp, C.c_float, vp, vp, C.c_int]),
        "sb_cg_update_p_launch_f32": (None, [u32, vp]),
        "sb_cg_update_r_launch_f32": (None, [u32, vp]),
        "sb_dot_l1_launch_f32": (None, [u32, vp]),
        "sb_stream_launch_f32": (None, [u32, vp]),
        # restarted GMRES(m)
        "sb_gmres_create": (vp, [vp, vp, vp, vp, C.c_int]),
        "sb_gmres_free": (None, [vp]),
        "sb_gmres_set_fused": (None, [vp, C.c_int]),
        "sb_gmres_restart": (C.c_int, [vp]),
        "sb_gmres_launches_per_step": (C.c_int, [vp, C.c_int]),
        "sb_gmres_solve": (C.c_int, [vp, C.c_int, C.c_double]),
        "sb_gmres_start": (None, [vp, C.c_int, C.c_double]),
        "sb_gmres_run_steps": (None, [vp, C.c_int]),
        "sb_gmres_finish": (C.c_int, [vp]),
        "sb_gmres_history": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "sb_gmres_solution": (None, [vp, vp]),
        "sb_gmres_check_residual": (C.c_double, [vp]),
        "sb_gmres_loop_ms": (C.c_double, [vp]),
        "sb_gmres_counters": (None, [vp, vp]),
        "sb_multidot": (None, [u32, C.c_int, vp, C.c_size_t, vp, vp]),
        "sb_multiaxpy_sub": (None, [u32, C.c_int, vp, C.c_size_t, vp, vp]),
        "sb_debug_sqrt_div": (None, [u32, vp, vp, vp, vp]),
        # batched CG
        "sb_spmmv_native": (None, [vp, C.c_int, vp, vp]),
        "sb_spmmv_native_dot": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "sb_block_interleave": (None, [vp, C.c_int, vp, vp]),
        "sb_block_deinterleave": (None, [vp, C.c_int, vp, vp]),
        "sb_matrix_spmmv_bytes": (C.c_double, [vp, C.c_int]),
        "sb_cgb_create": (vp, [vp, vp, C.c_int, vp, vp]),
        "sb_cgb_free": (None, [vp]),
        "sb_cgb_nrhs": (C.c_int, [vp]),
        "sb_cgb_launches_per_body": (C.c_int, [vp]),
        "sb_cgb_solve": (C.c_int, [vp, C.c_int, C.c_double]),
        "sb_cgb_start": (None, [vp, C.c_int, C.c_double]),
        "sb_cgb_run_iters": (None, [vp, C.c_int]),
        "sb_cgb_finish": (C.c_int, [vp]),
        "sb_cgb_iterations": (C.c_int, [vp, C.c_int]),
        "sb_cgb_history": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "sb_cgb_solution": (None, [vp, C.c_int, vp]),
        "sb_cgb_check_residual": (C.c_double, [vp, C.c_int]),
        "sb_cgb_loop_ms": (C.c_double, [vp]),
        "sb_cgb_counters": (None, [vp, C.c_int, vp]),
        "sb_block_vec_native": (None, [C.c_int, C.c_int, u32, vp, vp, vp, vp, vp, vp]),
        "sb_block_vec_launch": (None, [u32, vp]),
        "sb_cgb_update_p_native": (None, [C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, C.c_int]),
        "sb_cgb_x_finalize_native": (None, [C.c_int, u32, vp, vp, vp, vp]),
        "sb_cgb_rows_launch": (None, [u32, vp]),
        "sb_gmres_group_launch": (None, [u32, vp]),
        "sb_gmres_scale_launch": (None, [u32, vp]),
        "sb_gmres_step_launch": (None, [u32, vp]),
        "sb_gmres_multidot_native": (C.c_int, [u32, C.c_int, vp, C.c_size_t, vp, vp, C.c_int]),
        "sb_gmres_finish_dots_native": (C.c_int, [u32, C.c_int, vp, C.c_size_t, C.c_int, vp, vp, vp, vp, C.c_int]),
        "sb_gmres_project_native": (C.c_int, [C.c_int, u32, C.c_int, vp, C.c_size_t, vp, vp, vp, C.c_int]),
        "sb_gmres_multiadd_native": (C.c_int, [u32, C.c_int, C.c_double, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int]),
        "sb_gmres_scale_native": (C.c_int, [u32, C.c_int, C.c_double, vp, vp, vp, vp, vp, vp, vp, C.c_int]),
        "sb_gmres_rr_native": (C.c_int, [C.c_int, u32, vp, C.c_int, vp, vp, C.c_int, vp, vp]),
        "sb_gmres_step_native": (C.c_int, [C.c_int, C.c_int, C.c_double, u32, C.c_int, C.c_int, u32, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sb_gmres_backsolve_native": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        # CG with a diagonal preconditioner
        "sb_matrix_diagonal": (None, [vp, vp]),
        "sb_pcg_create": (vp, [vp, vp, vp, vp, vp]),
        "sb_pcg_free": (None, [vp]),
        "sb_pcg_solve": (C.c_int, [vp, C.c_int, C.c_double]),
        "sb_pcg_start": (None, [vp, C.c_int, C.c_double]),
        "sb_pcg_run_iters": (None, [vp, C.c_int]),
        "sb_pcg_finish": (C.c_int, [vp]),
        "sb_pcg_history": (C.c_int, [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]),
        "sb_pcg_solution": (None, [vp, vp]),
        "sb_pcg_check_residual": (C.c_double, [vp]),
        "sb_pcg_dinv": (None, [vp, vp]),
        "sb_pcg_launches_per_body": (C.c_int, [vp]),
        "sb_pcg_loop_ms": (C.c_double, [vp]),
        "sb_pcg_counters": (None, [vp, vp]),
        "sb_pcg_update_r_native": (None, [u32, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_update_r_launch": (None, [u32, vp]),
        "sb_pcg_collectives_per_body": (C.c_int, [vp]),
        "sb_pcg_local_reduce_native": (None, [u32, C.c_int, C.c_int, vp, vp, vp]),
        "sb_pcg_create_sgs": (vp, [vp, vp, vp, vp]),
        "sb_pcg_precond": (C.c_int, [vp]),
        "sb_pcg_colours": (C.c_int, [vp]),
        "sb_pcg_colouring": (None, [vp, vp]),
        "sb_pcg_apply_precond": (None, [vp, vp, vp]),
        "sb_pcg_precond_bytes": (C.c_double, [vp]),
        "sb_pcg_apply_precond_ms": (C.c_double, [vp, C.c_int]),
        "sb_pcg_create_mg": (vp, [vp, vp, vp, vp, C.c_int, vp, vp]),
        "sb_pcg_levels": (C.c_int, [vp]),
        "sb_pcg_level_rows": (u32, [vp, C.c_int]),
        "sb_pcg_level_colours": (C.c_int, [vp, C.c_int]),
        "sb_pcg_create_mg_p": (vp, [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
        "sb_pcg_mg_fw_probe": (None, [vp, C.c_int, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_create_poly": (vp, [vp, vp, vp, vp, C.c_int, C.c_double, C.c_double]),
        "sb_pcg_poly_steps": (C.c_int, [vp]),
        "sb_pcg_poly_interval": (None, [vp, vp]),
        "sb_pcg_poly_coeffs": (None, [vp, vp]),
        "sb_pcg_poly_rowbound": (None, [vp, vp]),
        "sb_pcg_poly_update_r_native": (None, [u32, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_poly_step_native": (None, [u32, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_poly_step_launch": (None, [u32, vp]),
        "sb_pcg_create_mg_poly": (vp, [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_double]),
        "sb_pcg_mg_poly_level_steps": (C.c_int, [vp, C.c_int]),
        "sb_pcg_mg_poly_interval": (None, [vp, C.c_int, vp]),
        "sb_pcg_mg_poly_coeffs": (None, [vp, C.c_int, vp]),
        "sb_pcg_mg_poly_probe": (None, [vp, C.c_int, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_mg_poly_first_native": (None, [u32, C.c_int, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sb_pcg_mg_poly_first_launch": (None, [u32, vp]),
        # BiCGStab with a diagonal preconditioner
        "sb_bicgstab_create": (vp, [vp, vp, vp, vp, C.c_int, vp]),
        "sb_bicgstab_free": (None, [vp]),
        "sb_bicgstab_solve": (C.c_int, [vp, C.c_int, C.c_double]),
        "sb_bicgstab_start": (None, [vp, C.c_int, C.c_double]),
        "sb_bicgstab_run_iters": (None, [vp, C.c_int]),
        "sb_bicgstab_finish": (C.c_int, [vp]),
        "sb_bicgstab_history": (C.c_int, [vp, C.c_int, vp, C.c_int]),
        "sb_bicgstab_solution": (None, [vp, vp]),
        "sb_bicgstab_check_residual": (C.c_double, [vp]),
        "sb_bicgstab_dinv": (None, [vp, vp]),
        "sb_bicgstab_launches_per_body": (C.c_int, [vp]),
        "sb_bicgstab_loop_ms": (C.c_double, [vp]),
        "sb_bicgstab_counters": (None, [vp, vp]),
        "sb_bicgstab_update_p_native": (None, [u32, C.c_double, C.c_double, vp, vp, vp, vp, vp]),
        "sb_bicgstab_update_s_native": (None, [u32, C.c_double, vp, vp, vp, vp, vp]),
        "sb_bicgstab_dot2_native": (None, [u32, C.c_int, vp, vp, vp, vp]),
        "sb_bicgstab_update_xr_native": (None, [u32, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "sb_bicgstab_reduce_native": (None, [u32, vp, vp, vp]),
        "sb_bicgstab_launch": (None, [u32, vp]),
        # ... with the preconditioner plan of a borrowed sb_pcg handle
        "sb_bicgstab_create_pre": (vp, [vp, vp, vp, vp, vp]),
        "sb_gmres_create_pre": (vp, [vp, vp, vp, vp, C.c_int, vp]),
        "sb_gmres_create_dinv": (vp, [vp, vp, vp, vp, C.c_int, vp]),
        "sb_gmres_precond": (C.c_int, [vp]),
        "sb_gmres_dinv": (None, [vp, vp]),
        "sb_gmres_pre_scale_native": (None, [u32, C.c_int, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
        "sb_gmres_pre_multiupdate_native": (None, [u32, C.c_int, C.c_double, C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp]),
        "sb_gmres_pre_step_native": (None, [u32, C.c_int, C.c_double, C.c_int, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
        "sb_bicgstab_precond": (C.c_int, [vp]),
        "sb_bicgstab_plan_update_p_native": (None, [u32, C.c_int, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
        "sb_bicgstab_plan_update_s_native": (None, [u32, C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
        # Galerkin coarse operators on the device
        "sb_matrix_galerkin": (vp, [vp, u32, vp, vp, vp]),
        "sb_csr_rows": (u32, [vp]),
        "sb_csr_nnz": (C.c_uint64, [vp]),
        "sb_csr_copy": (None, [vp, vp, vp, vp]),
        "sb_csr_stats": (None, [vp, vp]),
        "sb_csr_free": (None, [vp]),
        # smoothed-aggregation prolongation from the matrix alone
        "sb_matrix_aggregate": (C.c_int, [vp, C.c_double, vp, vp, vp]),
        "sb_matrix_sa_prolongation": (vp, [vp, C.c_double, C.c_double, C.c_double, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


# include/sbhip.h: sb_transport
ALLREDUCE_FN = C.CFUNCTYPE(None, vp, vp, C.c_int)
EXCHANGE_FN = C.CFUNCTYPE(None, vp, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                          vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))


ALLGATHER_BYTES_FN = C.CFUNCTYPE(None, vp, vp, C.c_int, vp)


class TransportS(C.Structure):
    _fields_ = [("ctx", vp), ("allreduce", ALLREDUCE_FN), ("neighbour_exchange", EXCHANGE_FN),
                ("allgather_bytes", ALLGATHER_BYTES_FN)]


def init(device=None):
    """Select the GPU (LOCAL_RANK by default) and create the layer's stream."""
    L = load()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    if L.sb_device_count() == 0:
        raise RuntimeError("sparsebench_amd: no HIP device visible; the HIP path is the only "
                           "path (no CPU fallback)")
    L.sb_init(device)
    return L


def _hp(a):
    return a.ctypes.data_as(vp)


class DeviceVector:
    """A vector of doubles (or, dtype=np.float32, floats) in HBM owned through the C-ABI (sb_malloc / sb_free)."""

    def __init__(self, n, host=None, dtype=np.float64):
        self.L = load()
        self.n = int(n)
        self.dtype = np.dtype(dtype)
        self.isz = self.dtype.itemsize
        self.ptr = self.L.sb_malloc(max(self.n, 1) * self.isz)
        if host is not None:
            self.set(host)

    @classmethod
    def from_host(cls, a, dtype=np.float64):
        a = np.ascontiguousarray(a, dtype=dtype)
        return cls(len(a), a, dtype)

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert len(a) == self.n
        if self.n:
            self.L.sb_h2d(self.ptr, _hp(a), self.n * self.isz)

    def get(self):
        out = np.empty(self.n, dtype=self.dtype)
        if self.n:
            self.L.sb_d2h(_hp(out), self.ptr, self.n * self.isz)
        return out

    def zero(self):
        self.L.sb_memset(self.ptr, 0, self.n * self.isz)

    def free(self):
        if self.ptr:
            self.L.sb_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
