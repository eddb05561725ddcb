"""ctypes binding of the C ABI declared in include/l3k.h (l3ster_amd/lib/libl3k.so).

This is the reference-side binding a maintainer would write; it contains no compute.  The library
must be present: there is no Python / CPU fallback for the device entry points.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("L3K_LIB") or os.path.join(_HERE, "lib", "libl3k.so")

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_uint32_p = C.POINTER(C.c_uint32)
c_uint8_p = C.POINTER(C.c_uint8)


class KParams(C.Structure):
    _fields_ = [("dimension", C.c_int), ("n_equations", C.c_int), ("n_unknowns", C.c_int), ("n_fields", C.c_int),
                ("n_rhs", C.c_int)]


class AsmOpts(C.Structure):
    _fields_ = [("value_order", C.c_int), ("derivative_order", C.c_int), ("eval_strategy", C.c_int)]


class CgOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("max_iters", C.c_int), ("residual_scaling", C.c_int), ("check_every", C.c_int)]


class CgResult(C.Structure):
    _fields_ = [("achieved_tol", C.c_double), ("iterations", C.c_int), ("converged", C.c_int)]


class GmresOpts(C.Structure):
    """l3k_gmres_opts (IterSolverOpts with its restart fields, solve/SolverInterface.hpp:26-37)"""
    _fields_ = [("tol", C.c_double), ("max_iters", C.c_int), ("residual_scaling", C.c_int), ("check_every", C.c_int),
                ("max_restarts", C.c_int)]


class GmresResult(C.Structure):
    _fields_ = [("achieved_tol", C.c_double), ("estimate", C.c_double), ("orth_loss", C.c_double), ("iterations", C.c_int),
                ("restarts", C.c_int), ("converged", C.c_int), ("breakdown", C.c_int)]


class GmresInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("ld", C.c_int64), ("restart_length", C.c_int), ("bytes", C.c_size_t)]


class ChebOpts(C.Structure):
    """l3k_cheb_opts (Ifpack2ChebyshevPreconditioner::Options, solve/Ifpack2Preconditioners.hpp:107-118)"""
    _fields_ = [("degree", C.c_int), ("cond_est", C.c_double), ("max_power_iters", C.c_int), ("boost_factor", C.c_double),
                ("lambda_max", C.c_double)]


class ChebInfo(C.Structure):
    _fields_ = [("lambda_max", C.c_double), ("lambda_min", C.c_double), ("lambda_est", C.c_double), ("degree", C.c_int),
                ("power_iters", C.c_int), ("applies_per_call", C.c_int)]


class PmgLevel(C.Structure):
    """l3k_pmg_level: operator, smoother and element map (device int64, or NULL) of one p-multigrid level"""
    _fields_ = [("mf", C.c_void_p), ("smoother", C.c_void_p), ("d_elem_map", C.c_void_p)]


class PmgInfo(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("order", C.c_int * 8), ("n_dofs", C.c_int64 * 8), ("applies_per_cycle", C.c_int * 8)]


class TransferInfo(C.Structure):
    """l3k_transfer_info: orders and owned / ghost dof counts of the two levels of a transfer"""
    _fields_ = [("order_fine", C.c_int), ("order_coarse", C.c_int), ("n_owned_dofs_fine", C.c_int64),
                ("n_ghost_dofs_fine", C.c_int64), ("n_owned_dofs_coarse", C.c_int64), ("n_ghost_dofs_coarse", C.c_int64)]


class CsrInfo(C.Structure):
    """l3k_csr_info: what the validation pass of l3k_csr_create gathered"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("n_empty_rows", C.c_int64), ("max_row_len", C.c_int64),
                ("mean_row_len", C.c_double), ("lanes_per_row", C.c_int)]


class CholOpts(C.Structure):
    """l3k_chol_opts: the memory limit of the factor (0 = 8 GiB) and the block size (0 = chosen, 32 or 64)"""
    _fields_ = [("max_bytes", C.c_size_t), ("block", C.c_int)]


class CholInfo(C.Structure):
    """l3k_chol_info: sizes of the symbolic phase and the outcome of the last numeric factorisation"""
    _fields_ = [("n", C.c_int64), ("n_active", C.c_int64), ("n_blocks", C.c_int64), ("block", C.c_int), ("max_height", C.c_int64),
                ("factor_bytes", C.c_size_t), ("factor_flops", C.c_double), ("update_flops", C.c_double),
                ("n_bad_pivots", C.c_int64), ("first_bad_row", C.c_int64), ("factored", C.c_int)]


class TriOpts(C.Structure):
    """l3k_tri_opts (Ifpack2SGSOpts / Ifpack2IluKOpts, solve/Ifpack2Preconditioners.hpp:97-101,134-157): kind 0 = SGS, 1 = ILU(0)"""
    _fields_ = [("kind", C.c_int), ("damping", C.c_double), ("absolute_threshold", C.c_double), ("relative_threshold", C.c_double),
                ("fuse_rows", C.c_int)]


class TriInfo(C.Structure):
    """l3k_tri_info: sizes of the symbolic phase, the launch plan and the outcome of the last l3k_tri_factor"""
    _fields_ = [("n", C.c_int64), ("n_active", C.c_int64), ("nnz", C.c_int64), ("kind", C.c_int), ("lanes_per_row", C.c_int),
                ("n_levels_lower", C.c_int64), ("n_levels_upper", C.c_int64), ("max_level_rows", C.c_int64),
                ("n_launches_lower", C.c_int64), ("n_launches_upper", C.c_int64), ("bytes", C.c_size_t),
                ("n_bad_pivots", C.c_int64), ("first_bad_row", C.c_int64), ("factored", C.c_int)]


class GraphInfo(C.Structure):
    """l3k_graph_info: the statistics of the one readback of l3k_graph_create"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("n_empty_rows", C.c_int64), ("max_row_len", C.c_int64),
                ("n_rows_scratch", C.c_int64), ("workspace_bytes", C.c_int64), ("max_elems_per_node", C.c_int),
                ("lds_key_capacity", C.c_int)]


class AsmCondInfo(C.Structure):
    """l3k_asm_cond_info: the per-element store of a condensed assembled system and the pivot failures of its last end"""
    _fields_ = [("condensed", C.c_int), ("n_primary_nodes", C.c_int), ("n_internal_nodes", C.c_int), ("n_elems", C.c_int64),
                ("store_bytes", C.c_int64), ("n_failed", C.c_int64)]


class AsmInfo(C.Structure):
    """l3k_asm_info: sizes, state, entries outside the graph, the device pointers of the four arrays and the operator"""
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("n_missing", C.c_int64), ("ldr", C.c_size_t), ("n_rhs", C.c_int),
                ("state", C.c_int), ("d_row_ptr", C.c_void_p), ("d_col_ind", C.c_void_p), ("d_values", C.c_void_p),
                ("d_rhs", C.c_void_p), ("csr", C.c_void_p)]


class MfsInfo(C.Structure):
    """l3k_mfs_info: terms, owned rows, active and Dirichlet rows among them, columns, state of a sum of matrix-free terms"""
    _fields_ = [("n_terms", C.c_int64), ("n_rows", C.c_int64), ("n_active_rows", C.c_int64), ("n_dirichlet_rows", C.c_int64),
                ("n_rhs", C.c_int), ("finalized", C.c_int)]


class CsrDistInfo(C.Structure):
    """l3k_csr_dist_info: the sizes of a distributed CSR operator, its three row lists and its local operator"""
    _fields_ = [("n_owned", C.c_int64), ("n_ghost", C.c_int64), ("n_interior_rows", C.c_int64), ("n_border_rows", C.c_int64),
                ("n_ghost_rows", C.c_int64), ("d_interior_rows", C.c_void_p), ("d_border_rows", C.c_void_p),
                ("d_ghost_rows", C.c_void_p), ("local", C.c_void_p)]


class AsmDistInfo(C.Structure):
    """l3k_asm_dist_info: the sizes of a partitioned assembled system and, once it is closed, its distributed operator"""
    _fields_ = [("n_owned", C.c_int64), ("n_ghost", C.c_int64), ("dist", C.c_void_p)]


class VtkOpts(C.Structure):
    """l3k_vtk_opts: text bytes per pipeline chunk of the ParaView export (0 = default)"""
    _fields_ = [("chunk_bytes", C.c_size_t)]


class VtkInfo(C.Structure):
    """l3k_vtk_info: points, sub-cells, connectivity entries, raw and encoded bytes of Position / connectivity / offsets / types"""
    _fields_ = [("dim", C.c_int), ("order", C.c_int), ("n_points", C.c_int64), ("n_cells", C.c_int64), ("n_conn", C.c_int64),
                ("raw_bytes", C.c_uint64 * 4), ("encoded_bytes", C.c_uint64 * 4), ("chunk_bytes", C.c_size_t),
                ("store_bytes", C.c_int)]


class MeshDesc(C.Structure):
    _fields_ = [("dim", C.c_int), ("order", C.c_int), ("n_elems", C.c_int64), ("n_interior_elems", C.c_int64),
                ("elem_nodes", c_uint32_p), ("elem_verts", c_double_p), ("n_owned_nodes", C.c_int64),
                ("n_ghost_nodes", C.c_int64), ("dofs_per_node", C.c_int), ("dirichlet", c_uint8_p)]


class HostMeshView(C.Structure):
    _fields_ = [("dim", C.c_int), ("order", C.c_int), ("n_elems", C.c_int64), ("n_interior_elems", C.c_int64),
                ("n_owned_nodes", C.c_int64), ("n_ghost_nodes", C.c_int64), ("global_node_base", C.c_int64),
                ("n_global_nodes", C.c_int64), ("elem_nodes", c_uint32_p), ("elem_verts", c_double_p),
                ("node_grid_id", c_int64_p), ("node_boundary", c_uint8_p), ("n_nbrs", C.c_int), ("nbr_rank", c_int_p),
                ("send_offsets", c_int64_p), ("send_nodes", c_int32_p), ("ghost_offsets", c_int64_p),
                ("elem_boundary", c_uint8_p), ("ghost_global_id", c_int64_p)]


c_uint64_p = C.POINTER(C.c_uint64)
c_uint16_p = C.POINTER(C.c_uint16)


class HaloTransport(C.Structure):
    """l3k_halo_transport: group begin / send / recv / group end (+ destroy) over device pointers and a HIP stream."""
    GROUP_BEGIN = C.CFUNCTYPE(C.c_int, C.c_void_p)
    SEND = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    RECV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
    GROUP_END = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
    DESTROY = C.CFUNCTYPE(None, C.c_void_p)
    _fields_ = [("user", C.c_void_p), ("group_begin", GROUP_BEGIN), ("send", SEND), ("recv", RECV), ("group_end", GROUP_END),
                ("destroy", DESTROY)]


class MeshFileElems(C.Structure):
    _fields_ = [("n", C.c_size_t), ("nodes", c_uint64_p), ("verts", c_double_p), ("ids", c_uint64_p)]


class MeshFileDomain(C.Structure):
    _fields_ = [("id", C.c_uint16), ("hex", MeshFileElems), ("quad", MeshFileElems), ("line", MeshFileElems)]


class MeshFilePartDesc(C.Structure):
    _fields_ = [("order", C.c_int), ("n_domains", C.c_size_t), ("domains", C.POINTER(MeshFileDomain)),
                ("nodes_begin", C.c_uint64), ("n_owned_nodes", C.c_size_t), ("n_boundary_ids", C.c_size_t),
                ("boundary_ids", c_uint16_p)]


class Tuning(C.Structure):
    """l3k_tuning: the launch-route settings of a context (include/l3k.h)"""
    _fields_ = [("generic_below", C.c_int64), ("static_deal", C.c_int), ("waves_per_cu", C.c_int), ("no_affine", C.c_int),
                ("column_by_column", C.c_int), ("assemble_dense", C.c_int), ("assemble_two_launches", C.c_int),
                ("scatter_per_entry", C.c_int), ("assemble_direct_store", C.c_int), ("assemble_sub_batch", C.c_int), ("assemble_no_symmetrise", C.c_int)]


# every symbol include/l3k.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SIGNATURES = {
    "l3k_version": (C.c_int, []),
    "l3k_last_error": (C.c_char_p, []),
    "l3k_gll_nodes": (C.c_int, [C.c_int, c_double_p]),
    "l3k_gl_rule": (C.c_int, [C.c_int, c_double_p, c_double_p]),
    "l3k_n_qps1d": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "l3k_basis_1d": (C.c_int, [C.c_int, C.c_int, c_double_p, c_double_p]),
    "l3k_colloc_deriv": (C.c_int, [C.c_int, c_double_p]),
    "l3k_interp_1d": (C.c_int, [C.c_int, C.c_int, c_double_p]),
    "l3k_kernel_info": (C.c_int, [C.c_int, C.POINTER(KParams), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]),
    "l3k_plugin_load": (C.c_int, [C.c_char_p]),
    "l3k_instance_count": (C.c_int, []),
    "l3k_instance_info": (C.c_int, [C.c_int, c_int_p, c_int_p, c_int_p, c_int_p]),
    "l3k_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "l3k_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "l3k_ctx_set_deterministic": (C.c_int, [_vp, C.c_int]),
    "l3k_ctx_set_reference_z0": (C.c_int, [_vp, C.c_int]),
    "l3k_ctx_get_tuning": (C.c_int, [_vp, C.POINTER(Tuning)]),
    "l3k_ctx_set_tuning": (C.c_int, [_vp, C.POINTER(Tuning)]),
    "l3k_mf_route": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    "l3k_last_fast_launch": (C.c_int, [C.POINTER(C.c_uint)]),
    "l3k_ctx_synchronize": (C.c_int, [_vp]),
    "l3k_ctx_destroy": (C.c_int, [_vp]),
    "l3k_mesh_create": (C.c_int, [_vp, C.POINTER(MeshDesc), C.POINTER(_vp)]),
    "l3k_mesh_destroy": (C.c_int, [_vp]),
    "l3k_mf_create": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, C.POINTER(AsmOpts), c_int_p, C.c_int,
                                C.POINTER(_vp)]),
    "l3k_mf_destroy": (C.c_int, [_vp]),
    "l3k_mf_set_fields": (C.c_int, [_vp, _vp, C.c_size_t]),
    "l3k_mf_set_time": (C.c_int, [_vp, C.c_double]),
    "l3k_mf_apply": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double, C.c_double]),
    "l3k_mf_scale": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_double]),
    "l3k_mf_apply_elems": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t,
                                     C.c_int, C.c_double, C.c_double]),
    "l3k_mf_dirichlet_rows": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double]),
    "l3k_pack_rows": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_int64, _vp]),
    "l3k_unpack_add_rows": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_size_t, C.c_int]),
    "l3k_mf_diag_rhs": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int]),
    "l3k_mf_dirichlet_finalize": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t]),
    "l3k_local_assemble": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "l3k_halo_unique_id": (C.c_int, [C.c_char_p]),
    "l3k_halo_create": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, c_int_p, c_int64_p, c_int32_p, c_int64_p,
                                  C.POINTER(_vp)]),
    "l3k_halo_create_transport": (C.c_int, [_vp, C.POINTER(HaloTransport), C.c_int, C.c_int, C.c_int, C.c_int, c_int_p, c_int64_p,
                                            c_int32_p, c_int64_p, C.POINTER(_vp)]),
    "l3k_inproc_group_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "l3k_inproc_group_destroy": (C.c_int, [_vp]),
    "l3k_inproc_transport": (C.c_int, [_vp, C.c_int, C.POINTER(HaloTransport)]),
    "l3k_halo_destroy": (C.c_int, [_vp]),
    "l3k_halo_n_ghost_dofs": (C.c_int64, [_vp]),
    "l3k_halo_import": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t]),
    "l3k_halo_export_add": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, C.c_size_t]),
    "l3k_halo_timing_begin": (C.c_int, [_vp, C.c_int]),
    "l3k_halo_timing_get": (C.c_int, [_vp, C.c_int, c_double_p]),
    "l3k_mf_apply_dist": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double, C.c_double]),
    "l3k_assembled_scatter": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int,
                                        c_int64_p]),
    "l3k_local_assemble_tiled": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "l3k_assemble_global": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, c_int64_p]),
    "l3k_condense_local": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "l3k_condense_global": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, c_int64_p]),
    "l3k_condensed_recover": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, C.c_size_t]),
    "l3k_bnd_create": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, C.POINTER(AsmOpts), c_int_p, C.c_int, C.c_int64,
                                 c_int64_p, c_uint8_p, C.POINTER(_vp)]),
    "l3k_bnd_destroy": (C.c_int, [_vp]),
    "l3k_bnd_set_fields": (C.c_int, [_vp, _vp, C.c_size_t]),
    "l3k_bnd_set_time": (C.c_int, [_vp, C.c_double]),
    "l3k_bnd_apply": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int,
                                C.c_double]),
    "l3k_bnd_diag_rhs": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t]),
    "l3k_mf_attach_boundary": (C.c_int, [_vp, _vp]),
    "l3k_bnd_local_assemble": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "l3k_bnd_assemble_global": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, c_int64_p]),
    "l3k_mf_assemble_boundary": (C.c_int, [_vp, C.c_int]),
    "l3k_residual_info": (C.c_int, [C.c_int, C.POINTER(KParams), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]),
    "l3k_integrate": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, C.POINTER(AsmOpts), _vp, C.c_size_t, C.c_double,
                                C.c_int, C.c_int64, c_int64_p, c_uint8_p, c_double_p]),
    "l3k_values_at_nodes": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_double, C.c_int64, c_int64_p,
                                      c_uint8_p, c_int_p, _vp, _vp]),
    "l3k_average_values": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_update_solution": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_int, c_int_p, c_int_p, _vp, C.c_size_t,
                                      C.c_int]),
    "l3k_jacobi_inverse": (C.c_int, [_vp, _vp, C.c_int64, C.c_double, C.c_double, _vp]),
    "l3k_pcg_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_pcg_solve_cols": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_cg_init": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_cg_dot_pap": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_mf_apply_energy": (C.c_int, [_vp, _vp, _vp, _vp]),
    "l3k_mf_energy_begin": (C.c_int, [_vp, _vp]),
    "l3k_mf_energy_end": (C.c_int, [_vp, _vp, c_int_p]),
    "l3k_cg_update_z": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_cg_update_px": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_cheb_create": (C.c_int, [_vp, _vp, C.POINTER(ChebOpts), C.POINTER(_vp)]),
    "l3k_cheb_info_get": (C.c_int, [_vp, C.POINTER(ChebInfo)]),
    "l3k_cheb_apply": (C.c_int, [_vp, _vp, _vp]),
    "l3k_cheb_destroy": (C.c_int, [_vp]),
    "l3k_pcg_solve_cheb": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_cheb_first": (C.c_int, [_vp, _vp, _vp, C.c_double, _vp, _vp, C.c_int64, _vp]),
    "l3k_cheb_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, C.c_int64, _vp]),
    "l3k_cg_update_rx": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_cg_update_p": (C.c_int, [_vp, _vp, _vp, C.c_int64, _vp]),
    "l3k_pmg_create": (C.c_int, [_vp, C.c_int, C.POINTER(PmgLevel), C.POINTER(_vp)]),
    "l3k_pmg_info_get": (C.c_int, [_vp, C.POINTER(PmgInfo)]),
    "l3k_pmg_prolong": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int]),
    "l3k_pmg_restrict": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "l3k_pmg_apply": (C.c_int, [_vp, _vp, _vp]),
    "l3k_pmg_destroy": (C.c_int, [_vp]),
    "l3k_pcg_solve_pmg": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_transfer_create": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "l3k_transfer_info_get": (C.c_int, [_vp, C.POINTER(TransferInfo)]),
    "l3k_transfer_prolong": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "l3k_transfer_restrict": (C.c_int, [_vp, _vp, _vp, _vp]),
    "l3k_transfer_destroy": (C.c_int, [_vp]),
    "l3k_pmg_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64]),
    "l3k_csr_create": (C.c_int, [_vp, C.c_int64, _vp, _vp, _vp, C.c_int, C.POINTER(_vp)]),
    "l3k_csr_info_get": (C.c_int, [_vp, C.POINTER(CsrInfo)]),
    "l3k_csr_apply": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double, C.c_double]),
    "l3k_csr_apply_energy": (C.c_int, [_vp, _vp, _vp, _vp]),
    "l3k_csr_diag": (C.c_int, [_vp, _vp, C.c_double, C.c_double, _vp]),
    "l3k_csr_dirichlet": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int]),
    "l3k_csr_destroy": (C.c_int, [_vp]),
    "l3k_csr_pcg_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_csr_pcg_solve_cols": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, _vp, C.POINTER(CgOpts),
                                         C.POINTER(CgResult)]),
    "l3k_csr_cheb_create": (C.c_int, [_vp, _vp, C.POINTER(ChebOpts), C.POINTER(_vp)]),
    "l3k_csr_pcg_solve_cheb": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_chol_create": (C.c_int, [_vp, C.POINTER(CholOpts), C.POINTER(_vp)]),
    "l3k_chol_factor": (C.c_int, [_vp]),
    "l3k_chol_solve": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int]),
    "l3k_chol_info_get": (C.c_int, [_vp, C.POINTER(CholInfo)]),
    "l3k_chol_destroy": (C.c_int, [_vp]),
    "l3k_chol_order": (C.c_int, [C.c_int64, c_int64_p, c_int32_p, c_int32_p, c_int32_p, c_int_p, c_int64_p, C.POINTER(C.c_size_t)]),
    "l3k_graph_create": (C.c_int, [_vp, C.c_int, c_int_p, C.c_int, C.POINTER(_vp)]),
    "l3k_graph_info_get": (C.c_int, [_vp, C.POINTER(GraphInfo)]),
    "l3k_graph_fill": (C.c_int, [_vp, _vp, _vp]),
    "l3k_graph_destroy": (C.c_int, [_vp]),
    "l3k_asm_element_systems": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "l3k_asm_side_systems": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "l3k_asm_create": (C.c_int, [_vp, C.c_int, c_int_p, C.c_int, C.c_size_t, C.POINTER(_vp)]),
    "l3k_asm_begin": (C.c_int, [_vp]),
    "l3k_asm_add_domain": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64]),
    "l3k_asm_add_boundary": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64]),
    "l3k_asm_end": (C.c_int, [_vp, _vp, C.c_size_t]),
    "l3k_asm_info_get": (C.c_int, [_vp, C.POINTER(AsmInfo)]),
    "l3k_asm_destroy": (C.c_int, [_vp]),
    "l3k_asm_create_condensed": (C.c_int, [_vp, C.c_int, c_int_p, C.c_int, C.c_size_t, C.POINTER(_vp)]),
    "l3k_asm_cond_info_get": (C.c_int, [_vp, C.POINTER(AsmCondInfo)]),
    "l3k_asm_recover": (C.c_int, [_vp, _vp, C.c_size_t]),
    "l3k_asm_schur_updates": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "l3k_mfs_create": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "l3k_mfs_add_domain": (C.c_int, [_vp, _vp]),
    "l3k_mfs_add_boundary": (C.c_int, [_vp, _vp]),
    "l3k_mfs_finalize": (C.c_int, [_vp]),
    "l3k_mfs_info_get": (C.c_int, [_vp, C.POINTER(MfsInfo)]),
    "l3k_mfs_active": (C.c_int, [_vp, _vp]),
    "l3k_mfs_destroy": (C.c_int, [_vp]),
    "l3k_mfs_apply": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double, C.c_double]),
    "l3k_mfs_scale": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_double]),
    "l3k_mfs_apply_elems": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t, _vp, C.c_size_t,
                                      C.c_int, C.c_double, C.c_double]),
    "l3k_mfs_dirichlet_rows": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double]),
    "l3k_mfs_diag_rhs": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int]),
    "l3k_mfs_jacobi_inverse": (C.c_int, [_vp, _vp, C.c_double, C.c_double, _vp]),
    "l3k_mfs_apply_energy": (C.c_int, [_vp, _vp, _vp, _vp]),
    "l3k_mfs_pcg_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_mfs_pcg_solve_cols": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, _vp, C.POINTER(CgOpts),
                                         C.POINTER(CgResult)]),
    "l3k_mfs_cheb_create": (C.c_int, [_vp, _vp, C.POINTER(ChebOpts), C.POINTER(_vp)]),
    "l3k_mfs_pcg_solve_cheb": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_csr_dist_create": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(_vp)]),
    "l3k_csr_dist_info_get": (C.c_int, [_vp, C.POINTER(CsrDistInfo)]),
    "l3k_csr_dist_apply": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_double, C.c_double]),
    "l3k_csr_dist_diag": (C.c_int, [_vp, _vp, C.c_double, C.c_double, _vp]),
    "l3k_csr_dist_destroy": (C.c_int, [_vp]),
    "l3k_halo_allreduce_sum": (C.c_int, [_vp, _vp, C.c_int]),
    "l3k_csr_dist_apply_energy": (C.c_int, [_vp, _vp, _vp, _vp]),
    "l3k_pcg_solve_dist": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_csr_dist_pcg_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_cheb_create_dist": (C.c_int, [_vp, _vp, _vp, C.POINTER(ChebOpts), C.POINTER(_vp)]),
    "l3k_csr_dist_cheb_create": (C.c_int, [_vp, _vp, C.POINTER(ChebOpts), C.POINTER(_vp)]),
    "l3k_csr_dirichlet_dist": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_int64]),
    "l3k_asm_create_dist": (C.c_int, [_vp, _vp, C.c_int, c_int_p, C.c_int, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "l3k_asm_dist_info_get": (C.c_int, [_vp, C.POINTER(AsmDistInfo)]),
    "l3k_cube_partition_create": (C.c_int, [c_int_p, C.c_int, c_int_p, C.c_int, C.c_double, C.POINTER(_vp)]),
    "l3k_square_mesh_create": (C.c_int, [c_int_p, C.c_int, C.c_double, C.POINTER(_vp)]),
    "l3k_hostmesh_destroy": (C.c_int, [_vp]),
    "l3k_hostmesh_view_get": (C.c_int, [_vp, C.POINTER(HostMeshView)]),
    "l3k_elevate_order": (C.c_int, [_vp, C.c_int64, c_uint32_p, C.c_int64, C.c_int, c_uint32_p, c_int64_p, c_int64_p]),
    "l3k_elevate_order_quads": (C.c_int, [_vp, C.c_int64, c_uint32_p, C.c_int64, C.c_int, c_uint32_p, c_int64_p, c_int64_p]),
    "l3k_boundary_match": (C.c_int, [_vp, C.c_int, C.c_int64, c_uint32_p, C.c_int64, c_uint32_p, c_int64_p, c_uint8_p, c_int64_p,
                                     c_int64_p]),
    "l3k_periodic_match": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int64, c_uint32_p, c_double_p, C.c_int64, c_int64_p, c_uint8_p,
                                     C.c_int64, c_int64_p, c_uint8_p, c_double_p, C.c_double, c_uint32_p, c_uint32_p, c_int64_p,
                                     c_int64_p, c_int64_p, c_int64_p]),
    "l3k_periodic_merge": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, c_uint32_p, c_uint32_p, C.c_int64, c_uint32_p, c_uint32_p,
                                     c_int64_p, c_int64_p, c_int64_p]),
    "l3k_results_save": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int64, c_double_p, C.c_size_t,
                                   C.c_int]),
    "l3k_results_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "l3k_results_load": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int64, c_int64_p, C.c_int64, c_double_p]),
    "l3k_meshfile_part_bytes": (C.c_int, [C.POINTER(MeshFilePartDesc), C.POINTER(C.c_size_t)]),
    "l3k_meshfile_save": (C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_size_t,
                                    C.POINTER(MeshFilePartDesc), C.c_int]),
    "l3k_meshfile_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t]),
    "l3k_meshfile_load": (C.c_int, [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(_vp)]),
    "l3k_meshfile_part_get": (C.c_int, [_vp, C.POINTER(MeshFilePartDesc)]),
    "l3k_meshfile_part_destroy": (C.c_int, [_vp]),
    "l3k_vtk_sizes": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(VtkInfo)]),
    "l3k_vtk_encode": (C.c_int, [_vp, _vp, C.c_uint64, _vp, C.c_uint64]),
    "l3k_vtk_create": (C.c_int, [_vp, C.POINTER(VtkOpts), C.POINTER(_vp)]),
    "l3k_vtk_info_get": (C.c_int, [_vp, C.POINTER(VtkInfo)]),
    "l3k_vtk_destroy": (C.c_int, [_vp]),
    "l3k_vtk_export": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), c_int_p, c_int_p, _vp, C.c_size_t,
                                 C.c_int]),
    "l3k_vtk_pvtu_text": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), c_int_p, _vp, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "l3k_vtk_vtu_header_text": (C.c_int, [C.c_int64, C.c_int64, c_uint64_p, C.c_int, C.POINTER(C.c_char_p), c_int_p, _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    "l3k_gmres_create": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_size_t, C.POINTER(_vp)]),
    "l3k_gmres_info_get": (C.c_int, [_vp, C.POINTER(GmresInfo)]),
    "l3k_gmres_destroy": (C.c_int, [_vp]),
    **{name: (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(GmresOpts), C.POINTER(GmresResult)])
       for name in ("l3k_gmres_solve", "l3k_gmres_solve_cheb", "l3k_gmres_solve_pmg", "l3k_csr_gmres_solve", "l3k_csr_gmres_solve_cheb",
                    "l3k_mfs_gmres_solve", "l3k_mfs_gmres_solve_cheb")},
    "l3k_halo_reduce_reserve": (C.c_int, [_vp, C.c_int]),
    "l3k_halo_allreduce_sum_n": (C.c_int, [_vp, _vp, C.c_int]),
    "l3k_gmres_create_dist": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_size_t, C.POINTER(_vp)]),
    "l3k_gmres_solve_dist": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(GmresOpts), C.POINTER(GmresResult)]),
    "l3k_csr_dist_gmres_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(GmresOpts), C.POINTER(GmresResult)]),
    "l3k_gmres_multi_dot": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, _vp, C.c_int64, _vp]),
    "l3k_gmres_project": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, _vp, C.c_int64, _vp, _vp]),
    "l3k_gmres_combine": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp, _vp, C.c_int64, _vp]),
    "l3k_tri_create": (C.c_int, [_vp, C.POINTER(TriOpts), C.POINTER(_vp)]),
    "l3k_tri_factor": (C.c_int, [_vp]),
    "l3k_tri_apply": (C.c_int, [_vp, _vp, _vp]),
    "l3k_tri_solve_lower": (C.c_int, [_vp, _vp, _vp]),
    "l3k_tri_solve_upper": (C.c_int, [_vp, _vp, _vp]),
    "l3k_tri_values": (C.c_int, [_vp, _vp]),
    "l3k_tri_info_get": (C.c_int, [_vp, C.POINTER(TriInfo)]),
    "l3k_tri_destroy": (C.c_int, [_vp]),
    "l3k_tri_levels": (C.c_int, [C.c_int64, c_int64_p, c_int32_p, C.c_int, c_int32_p, c_int64_p]),
    "l3k_csr_pcg_solve_tri": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(CgOpts), C.POINTER(CgResult)]),
    "l3k_csr_gmres_solve_tri": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(GmresOpts), C.POINTER(GmresResult)]),
}

_lib = None


class L3KError(RuntimeError):
    pass


def load():
    """Loads libl3k.so; raises if it has not been built (python -m l3ster_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise L3KError(f"{LIB_PATH} is missing: build the HIP extension first (python -m l3ster_amd.build). "
                       "There is no CPU fallback for the device path.")
    # torch ships its own HIP runtime (same soname as /opt/rocm's, which libl3k.so names in its RUNPATH): whichever is
    # mapped first serves the whole process, and device memory / streams come from torch here -- so torch goes first
    try:
        import torch  # noqa: F401
    except ImportError:  # pure C-ABI use without torch: the system runtime
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise L3KError(f"libl3k error {rc}: {load().l3k_last_error().decode()}")
