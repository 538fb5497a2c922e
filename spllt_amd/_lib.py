"""ctypes binding of libspllt_hip.so (the C-ABI of include/spllt_iface.h + spllt_hip.h + spllt_hip_batch_mult.h).

The library is built in-tree by ``__graft_entry__.build()`` /
``make -C spllt_amd/csrc``.  There is no Python or CPU fallback for the
factorize path: if the shared library is missing this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libspllt_hip.so")


class spllt_options_t(C.Structure):
    """reference include/spllt_iface.h:14-31"""
    _fields_ = [(k, C.c_int) for k in (
        "print_level", "nrhs", "ncpu", "nb", "nemin", "prune_tree", "min_width_blas",
        "nb_min", "nb_max", "nrhs_min", "nrhs_max", "nb_linear_comp", "nrhs_linear_comp",
        "chunk")]

    @classmethod
    def default(cls):
        """SPLLT_OPTIONS_NULL(), reference include/spllt_iface.h:33-47"""
        return cls(print_level=0, nrhs=1, ncpu=1, nb=16, nemin=32, prune_tree=1,
                   min_width_blas=8, nb_min=32, nb_max=32, nrhs_min=1, nrhs_max=1,
                   nb_linear_comp=0, nrhs_linear_comp=0, chunk=10)


class spllt_inform_t(C.Structure):
    """reference include/spllt_iface.h:49-57"""
    _fields_ = [(k, C.c_int) for k in (
        "flag", "maxdepth", "num_factor", "num_flops", "num_nodes", "stat")]


class spllt_hip_sym_info_t(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "n", "nnz_a", "nnodes", "nbcol", "nblk", "arena", "nnz_l", "flops", "rlist_len")] + \
        [(k, C.c_int) for k in ("nb", "maxmn", "maxdepth", "nlevels")] + \
        [("ordering", C.c_char * 16)]


vp, vpp = C.c_void_p, C.POINTER(C.c_void_p)
i32, i64, u64, f64, cstr, long = C.c_int, C.c_int64, C.c_uint64, C.c_double, C.c_char_p, C.c_long
ip, i64p, dp, fp, longp = (C.POINTER(t) for t in (C.c_int, C.c_int64, C.c_double, C.c_float, C.c_long))
ipp, dpp = C.POINTER(ip), C.POINTER(dp)
opt, inf = C.POINTER(spllt_options_t), C.POINTER(spllt_inform_t)

# every symbol declared in include/spllt_iface.h and include/spllt_hip.h: name -> (restype, argtypes); device pointers
# go in as integers (vp)
_IFACE = {
    "spllt_analyse": (None, [vpp, vpp, opt, i32, ip, ip, inf, ip]),
    "spllt_factor": (None, [vp, vp, opt, i32, dp, inf]),
    "spllt_prepare_solve": (None, [vp, vp, i32, i32, longp, inf]),
    "spllt_set_mem_solve": (None, [vp, vp, i32, i32, long, dp, dp, inf]),
    "spllt_solve_workspace_size": (None, [vp, i32, i32, longp]),
    "spllt_solve": (None, [vp, opt, ip, i32, dp, inf, i32]),
    "spllt_solve_worker": (None, [vp, opt, ip, i32, dp, inf, i32, dp, long, vp]),
    "spllt_wait": (None, []),
    "spllt_chkerr": (None, [i32, ip, ip, dp, i32, dp, dp]),
    "spllt_deallocate_fkeep": (None, [vpp, ip]),
    "spllt_deallocate_akeep": (None, [vpp, ip]),
    "spllt_task_manager_deallocate": (None, [vpp, ip]),
    "spllt_task_manager_init": (None, [vpp]),
    "spllt_all": (None, [vpp, vpp, opt, i32, i32, i32, i32, ip, ip, dp, dp, dp, inf]),
}
_HIP = {
    "spllt_factor_diag_block_hip": (i32, [vp, i32, i32, vp, vp]),
    "spllt_solve_block_hip": (i32, [vp, i32, i32, vp, vp]),
    "spllt_update_block_hip": (i32, [vp, i32, i32, vp, i32, i32, vp, vp]),
    "spllt_update_between_hip": (i32, [vp, vp, i32, i32, vp, i32, vp, i32, vp, vp, i32]),
    "spllt_expand_buffer_hip": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, vp]),
    "spllt_scatter_block_hip": (i32, [vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, vp, i32]),
    "spllt_init_lfact_hip": (i32, [vp, vp, vp, vp, vp, i64]),
    "spllt_hip_analyse_ordered": (None, [vpp, vpp, opt, i32, ip, ip, inf, ip, ip]),
    "spllt_hip_sym_info": (i32, [vp, C.POINTER(spllt_hip_sym_info_t)]),
    "spllt_hip_sym_get": (i64, [vp, cstr, vp, i64]),
    "spllt_hip_set_engine": (i32, [vp, i32, i32, i32]),
    "spllt_hip_factor_dev": (None, [vp, vp, opt, i32, vp, inf]),
    "spllt_hip_wait": (i32, [vp]),
    "spllt_hip_get_factor": (i32, [vp, dp, i64]),
    "spllt_hip_device_factor": (vp, [vp]),
    "spllt_hip_factor_times": (i32, [vp, dp, dp, dp, ip]),
    "spllt_hip_program_get": (i64, [vp, cstr, vp, i64]),
    "spllt_hip_profile": (i32, [vp, dp, i32, fp, i32]),
    "spllt_hip_last_error": (cstr, [vp]),
    "spllt_hip_version": (cstr, []),
    "spllt_hip_set_partition": (i32, [vp, i32, i32, i64p]),
    "spllt_hip_set_exchange_buffer": (i32, [vp, vp]),
    "spllt_hip_continue": (i32, [vp]),
    "spllt_hip_pending_exchange": (i32, [vp]),
    "spllt_hip_partition_get": (i64, [vp, cstr, vp, i64]),
    "spllt_hip_solve_dev": (i32, [vp, vp, i32, i32, i32]),
    "spllt_hip_set_chain_block": (i32, [vp, i32]),
    "spllt_hip_engine_stream": (vp, [vp]),
    "spllt_hip_analyse_symbolic": (None, [vpp, vpp, opt, i32, ip, ip, inf, i32, ip, ip, i64p, ip, ip]),
    "spllt_hip_profile_in_program": (i32, [vp, dp, i32, fp, i32]),
    "spllt_hip_timeline": (i32, [vp, dp, i32, fp, i32]),
    "spllt_hip_read_rb": (i32, [cstr, i32, i32, ip, ip, ipp, ipp, dpp]),
    "spllt_hip_read_mm": (i32, [cstr, i32, i32, ip, ip, ipp, ipp, dpp]),
    "spllt_hip_free_matrix": (None, [ip, ip, dp]),
    "spllt_hip_set_communicator": (i32, [vp, vp]),
    "spllt_hip_last_flag": (i32, [vp]),
    "spllt_hip_debug": (i32, [cstr]),
    "spllt_hip_exchange_stream": (vp, [vp]),
    "spllt_hip_selected_inverse": (i32, [vp]),
    "spllt_hip_get_inverse": (i32, [vp, dp, i64]),
    "spllt_hip_device_inverse": (vp, [vp]),
    "spllt_hip_inverse_diag": (i32, [vp, dp, i32]),
    "spllt_hip_log_det": (i32, [vp, dp]),
    "spllt_hip_release_inverse": (i32, [vp]),
    "spllt_hip_solve_many": (i32, [vp, i32, dp, i64, i32]),
    "spllt_hip_solve_many_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_factor_batch": (i32, [vp, vp, i32, i32, vp, i64]),
    "spllt_hip_factor_batch_dev": (i32, [vp, vp, i32, i32, vp, i64]),
    "spllt_hip_batch_status": (i32, [vp, ip, ip, i32]),
    "spllt_hip_solve_batch": (i32, [vp, i32, vp, i64, i32]),
    "spllt_hip_solve_batch_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_get_factor_batch": (i32, [vp, i32, dp, i64]),
    "spllt_hip_device_factor_batch": (vp, [vp, i64p]),
    "spllt_hip_log_det_batch": (i32, [vp, dp]),
    "spllt_hip_batch_launches": (i32, [vp]),
    "spllt_hip_release_batch": (i32, [vp]),
    "spllt_hip_selected_inverse_batch": (i32, [vp]),
    "spllt_hip_get_inverse_batch": (i32, [vp, i32, dp, i64]),
    "spllt_hip_device_inverse_batch": (vp, [vp, i64p]),
    "spllt_hip_inverse_diag_batch": (i32, [vp, dp, i64]),
    "spllt_hip_inverse_on_pattern_batch": (i32, [vp, dp, i64]),
    "spllt_hip_batch_selinv_launches": (i32, [vp]),
    "spllt_hip_release_inverse_batch": (i32, [vp]),
    "spllt_hip_inverse_on_pattern": (i32, [vp, dp]),
    "spllt_hip_matvec": (i32, [vp, i32, dp, i32, dp, i64, dp, i64]),
    "spllt_hip_matvec_dev": (i32, [vp, i32, vp, i32, vp, i64, vp, i64, i32]),
    "spllt_hip_solve_refined": (i32, [vp, i32, dp, i32, dp, i64, i32, f64, i32, ip, dp]),
    "spllt_hip_solve_refined_dev": (i32, [vp, i32, vp, i32, vp, i64, i32, f64, i32, ip, dp]),
    "spllt_hip_release_refine": (i32, [vp]),
    "spllt_hip_updown": (i32, [vp, i32, ip, ip, dp, i32]),
    "spllt_hip_updown_plan": (i64, [vp, i32, ip, ip, ip, i64]),
    "spllt_hip_updown_info": (i32, [vp, i64p]),
    "spllt_hip_updown_time": (i32, [vp, dp]),
    "spllt_hip_solve_repro": (i32, [vp, i32, dp, i64, i32]),
    "spllt_hip_solve_repro_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_set_reproducible_solve": (i32, [vp, i32]),
    "spllt_hip_release_solve_repro": (i32, [vp]),
    "spllt_hip_factor_mult": (i32, [vp, i32, dp, i64, i32]),
    "spllt_hip_factor_mult_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_release_factor_mult": (i32, [vp]),
    "spllt_hip_sample": (i32, [vp, i32, dp, i64, i32, u64, u64, dp]),
    "spllt_hip_sample_dev": (i32, [vp, i32, vp, i64, i32, u64, u64, vp]),
    "spllt_hip_white_noise_dev": (i32, [vp, i32, vp, i64, u64, u64]),
    "spllt_hip_solve_sparse": (i32, [vp, i32, ip, ip, dp, i32, ip, dp, i64, i32]),
    "spllt_hip_solve_sparse_dev": (i32, [vp, i32, ip, ip, dp, i32, ip, vp, i64, i32]),
    "spllt_hip_gram_sparse": (i32, [vp, i32, ip, ip, dp, dp, i64]),
    "spllt_hip_solve_sparse_plan": (i32, [vp, i32, ip, ip, i32, ip, i32, ip, i64, ip, i64, i64p]),
    "spllt_hip_solve_sparse_info": (i32, [vp, i64p]),
    "spllt_hip_release_solve_sparse": (i32, [vp]),
    "spllt_hip_pattern_outer": (i32, [vp, i32, dp, i64, dp, i64, f64, dp]),
    "spllt_hip_pattern_outer_dev": (i32, [vp, i32, vp, i64, vp, i64, f64, vp]),
    "spllt_hip_pattern_outer_batch_dev": (i32, [vp, i32, i32, vp, i64, vp, i64, f64, vp, i64]),
    "spllt_hip_inverse_on_pattern_dev": (i32, [vp, vp]),
    "spllt_hip_inverse_on_pattern_batch_dev": (i32, [vp, vp, i64]),
    "spllt_hip_factor_serial": (i64, [vp, i32]),
    "spllt_hip_factor_adjoint_seed": (i32, [vp, i32, dp, dp, i64, f64, i32, i32]),
    "spllt_hip_factor_adjoint_seed_dev": (i32, [vp, i32, vp, vp, i64, f64, i32, i32]),
    "spllt_hip_set_factor_adjoint": (i32, [vp, dp, i64]),
    "spllt_hip_get_factor_adjoint": (i32, [vp, dp, i64]),
    "spllt_hip_device_factor_adjoint": (vp, [vp]),
    "spllt_hip_factor_adjoint": (i32, [vp, dp]),
    "spllt_hip_factor_adjoint_dev": (i32, [vp, vp]),
    "spllt_hip_release_factor_adjoint": (i32, [vp]),
}
PROTOTYPES = {**_IFACE, **_HIP}
# every symbol declared in include/spllt_hip_batch_mult.h: the batched factor products and samplers.  A table of its
# own, applied by load() after PROTOTYPES: the header is separate until the recorded ladder of the C boundary is
# regenerated (see the header), and PROTOTYPES stays what tests/test_abi.py ties to the two older headers.
u32 = C.c_uint32
_BATCH_MULT = {
    "spllt_hip_factor_mult_batch": (i32, [vp, i32, vp, i64, i32]),
    "spllt_hip_factor_mult_batch_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_white_noise_batch_dev": (i32, [vp, i32, vp, i64, u64, u64, u32, i32]),
    "spllt_hip_sample_batch": (i32, [vp, i32, vp, i64, i32, u64, u64, u32, i32, vp, i64]),
    "spllt_hip_sample_batch_dev": (i32, [vp, i32, vp, i64, i32, u64, u64, u32, i32, vp, i64]),
    "spllt_hip_release_factor_mult_batch": (i32, [vp]),
}
del u32
# every symbol declared in include/spllt_hip_batch_solve_many.h: the blocked solve for the members of a batch.  A
# table of its own for the same reason.
_BATCH_SOLVE_MANY = {
    "spllt_hip_solve_many_batch": (i32, [vp, i32, vp, i64, i32]),
    "spllt_hip_solve_many_batch_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_set_batch_blocked_solve": (i32, [vp, i32]),
    "spllt_hip_solve_many_batch_info": (i32, [vp, i64p]),
    "spllt_hip_release_solve_many_batch": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_batch_adjoint.h: the factor adjoint of the members of a batch.  A table
# of its own for the same reason.
_BATCH_ADJOINT = {
    "spllt_hip_factor_adjoint_seed_batch_dev": (i32, [vp, i32, vp, vp, i64, f64, i32, i32]),
    "spllt_hip_factor_adjoint_seed_batch": (i32, [vp, i32, dp, dp, i64, f64, i32, i32]),
    "spllt_hip_set_factor_adjoint_batch": (i32, [vp, dp, i64]),
    "spllt_hip_get_factor_adjoint_batch": (i32, [vp, i32, dp, i64]),
    "spllt_hip_device_factor_adjoint_batch": (vp, [vp, i64p]),
    "spllt_hip_factor_adjoint_batch_dev": (i32, [vp, vp, i64]),
    "spllt_hip_factor_adjoint_batch": (i32, [vp, dp, i64]),
    "spllt_hip_batch_adjoint_launches": (i32, [vp]),
    "spllt_hip_release_factor_adjoint_batch": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_batch_refine.h: the product A_b x and the refined solves of the members
# of a batch.  A table of its own for the same reason.
_BATCH_REFINE = {
    "spllt_hip_matvec_batch": (i32, [vp, i32, i32, dp, i64, i32, dp, i64, dp, i64]),
    "spllt_hip_matvec_batch_dev": (i32, [vp, i32, i32, vp, i64, i32, vp, i64, vp, i64, i32]),
    "spllt_hip_solve_refined_batch": (i32, [vp, i32, dp, i64, i32, dp, i64, i32, f64, i32, ip, dp]),
    "spllt_hip_solve_refined_batch_dev": (i32, [vp, i32, vp, i64, i32, vp, i64, i32, f64, i32, ip, dp]),
    "spllt_hip_solve_refined_batch_info": (i32, [vp, i64p]),
    "spllt_hip_release_refine_batch": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_constrain.h: hard linear constraints C x = e on the current factor.  A
# table of its own for the same reason.
_CONSTRAIN = {
    "spllt_hip_set_constraints": (i32, [vp, i32, dp, i64]),
    "spllt_hip_set_constraints_dev": (i32, [vp, i32, vp, i64]),
    "spllt_hip_constrain": (i32, [vp, i32, dp, i64, dp, i64, dp, i64]),
    "spllt_hip_constrain_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_solve_constrained": (i32, [vp, i32, dp, i64, dp, i64, dp, i64]),
    "spllt_hip_solve_constrained_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_sample_constrained": (i32, [vp, i32, dp, i64, u64, u64, dp, dp]),
    "spllt_hip_sample_constrained_dev": (i32, [vp, i32, vp, i64, u64, u64, vp, vp]),
    "spllt_hip_inverse_diag_constrained": (i32, [vp, dp, i32]),
    "spllt_hip_constraints_info": (i32, [vp, i64p, dp]),
    "spllt_hip_release_constraints": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_constrain_batch.h: hard linear constraints for the members of a batch.  A
# table of its own for the same reason.
u32 = C.c_uint32
_CONSTRAIN_BATCH = {
    "spllt_hip_set_constraints_batch": (i32, [vp, i32, dp, i64]),
    "spllt_hip_set_constraints_batch_dev": (i32, [vp, i32, vp, i64]),
    "spllt_hip_constrain_batch": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_constrain_batch_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_solve_constrained_batch": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_solve_constrained_batch_dev": (i32, [vp, i32, vp, i64, vp, i64, vp, i64]),
    "spllt_hip_sample_constrained_batch": (i32, [vp, i32, vp, i64, u64, u64, u32, i32, vp, i64, vp]),
    "spllt_hip_sample_constrained_batch_dev": (i32, [vp, i32, vp, i64, u64, u64, u32, i32, vp, i64, vp]),
    "spllt_hip_inverse_diag_constrained_batch": (i32, [vp, dp, i64]),
    "spllt_hip_constraints_batch_info": (i32, [vp, i64p, dp, i64]),
    "spllt_hip_release_constraints_batch": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_batch_repro.h: the bit-reproducible batch.  A table of its own for the
# same reason.
_BATCH_REPRO = {
    "spllt_hip_set_batch_reproducible": (i32, [vp, i32]),
    "spllt_hip_solve_repro_batch": (i32, [vp, i32, vp, i64, i32]),
    "spllt_hip_solve_repro_batch_dev": (i32, [vp, i32, vp, i64, i32, i32]),
    "spllt_hip_batch_repro_info": (i32, [vp, i64p]),
    "spllt_hip_release_batch_repro": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_updown_batch.h: the low-rank update / downdate of the factors of a
# batch.  A table of its own for the same reason.
_BATCH_UPDOWN = {
    "spllt_hip_updown_batch": (i32, [vp, i32, ip, ip, vp, i64, i32]),
    "spllt_hip_updown_batch_dev": (i32, [vp, i32, ip, ip, vp, i64, i32]),
    "spllt_hip_updown_batch_info": (i32, [vp, i64p]),
    "spllt_hip_updown_batch_time": (i32, [vp, dp]),
    "spllt_hip_release_updown_batch": (i32, [vp]),
}
# every symbol declared in include/spllt_hip_solve_sparse_batch.h: sparse right-hand sides, selected outputs and
# B^T A_b^-1 B for the members of a batch.  A table of its own for the same reason.
_SOLVE_SPARSE_BATCH = {
    "spllt_hip_solve_sparse_batch": (i32, [vp, i32, ip, ip, dp, i64, i32, ip, dp, i64, i32]),
    "spllt_hip_solve_sparse_batch_dev": (i32, [vp, i32, ip, ip, dp, i64, i32, ip, vp, i64, i32]),
    "spllt_hip_gram_sparse_batch": (i32, [vp, i32, ip, ip, dp, i64, dp, i64]),
    "spllt_hip_gram_sparse_batch_dev": (i32, [vp, i32, ip, ip, dp, i64, vp, i64]),
    "spllt_hip_solve_sparse_batch_info": (i32, [vp, i64p]),
    "spllt_hip_release_solve_sparse_batch": (i32, [vp]),
}
del u32
del vp, vpp, i32, i64, u64, f64, cstr, long, ip, i64p, dp, fp, longp, ipp, dpp, opt, inf   # (names of the table only)
IFACE_SYMBOLS = list(_IFACE)
HIP_SYMBOLS = list(_HIP)
BATCH_MULT_SYMBOLS = list(_BATCH_MULT)
BATCH_SOLVE_MANY_SYMBOLS = list(_BATCH_SOLVE_MANY)
BATCH_ADJOINT_SYMBOLS = list(_BATCH_ADJOINT)
BATCH_REFINE_SYMBOLS = list(_BATCH_REFINE)
CONSTRAIN_SYMBOLS = list(_CONSTRAIN)
CONSTRAIN_BATCH_SYMBOLS = list(_CONSTRAIN_BATCH)
BATCH_REPRO_SYMBOLS = list(_BATCH_REPRO)
BATCH_UPDOWN_SYMBOLS = list(_BATCH_UPDOWN)
SOLVE_SPARSE_BATCH_SYMBOLS = list(_SOLVE_SPARSE_BATCH)

_lib = None


def load():
    """Load libspllt_hip.so (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C spllt_amd/csrc`. spllt_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for table in (PROTOTYPES, _BATCH_MULT, _BATCH_SOLVE_MANY, _BATCH_ADJOINT, _BATCH_REFINE, _CONSTRAIN, _CONSTRAIN_BATCH,
                  _BATCH_REPRO, _BATCH_UPDOWN, _SOLVE_SPARSE_BATCH):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib
