"""ctypes binding of liblo_amd.so (the C ABI declared in include/lo_amd.h).

This is the ONLY compute backend of the package: there is no CPU or eager-PyTorch fallback.  If the
shared library is missing or a tensor is not a contiguous fp32 HIP tensor the call raises.
PyTorch is used for device memory (torch.empty workspaces through the caching allocator) and for the
current HIP stream only.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblo_amd.so")
_lib = None

LO_OP_LOWRANK_DIAG, LO_OP_DENSE_DIAG, LO_OP_KRON_DIAG, LO_OP_CALLBACK, LO_OP_SUM = 0, 1, 2, 3, 4
LO_MAX_TERMS = 4
LO_OP_SKI_DIAG, LO_OP_TOEPLITZ_DIAG = 5, 6
LO_TOEPLITZ_MAX_M = 16384
LO_OP_HADAMARD_DIAG = 7
LO_HADAMARD_MAX_RANK = 128
LO_OP_MASKED = 8
LO_OP_SKI_GRID_DIAG = 9
LO_SKI_GRID_MAX_AXIS = 1024
LO_SKI_GRID_MAX_M = 4194304
LO_OP_SKI_SUM_DIAG = 16
LO_SKI_SUM_MAX_TERMS = 64
LO_OP_TOEPLITZ_KRON_DIAG = 10
LO_KRON_EIG_MAX_SMALL, LO_KRON_EIG_MAX_COLS = 16, 256
LO_OP_KERNEL_DIAG = 11
LO_KERNEL_MAX_DIM = 32
LO_KERNEL_RBF, LO_KERNEL_MATERN12, LO_KERNEL_MATERN32, LO_KERNEL_MATERN52 = 0, 1, 2, 3
LO_OP_KERNEL_SUM_DIAG = 12
LO_KERNEL_MAX_TERMS = 4
LO_OP_KERNEL_KRON_DIAG = 13
LO_KERNEL_KRON_MAX_TASKS = 8
LO_OP_KERNEL_GRAD_DIAG = 14
LO_KERNEL_GRAD_MAX_DIM = 16
LO_OP_KERNEL_TASK_DIAG = 15
LO_KERNEL_TASK_MAX_TASKS = 8
LO_OP_KERNEL_LMC_DIAG = 17
LO_OP_KERNEL_PARAM_DIAG = 18
LO_KERNEL_RQ, LO_KERNEL_PERIODIC = 16, 17
LO_KERNEL_PARAM_MAX_DIM = 32
LO_OP_KERNEL_SM_DIAG = 19
LO_KERNEL_SM_MAX_DIM, LO_KERNEL_SM_MAX_MIX = 16, 16
LO_DIAG_NONE, LO_DIAG_FULL, LO_DIAG_CONST = 0, 1, 2
LO_BLOCK_DIAG, LO_BLOCK_INTERLEAVED, LO_BLOCK_SUM = 0, 1, 2
LO_EIGH_MAX_N = 1024
ABI_VERSION = 40

LO_ERR_UNSUPPORTED = -4
LO_FUSED_OK, LO_FUSED_EARLY_STOP, LO_FUSED_CONTINUE, LO_FUSED_TIMEOUT = 0, 1, 2, 3
_ERR = {-1: "bad argument", -2: "HIP launch/runtime failure", -3: "workspace too small", -4: "unsupported shape"}

class HipExtensionError(RuntimeError):
    pass


STOP_REDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))


class OpDesc(C.Structure):
    pass


OpDesc._fields_ = [("kind", C.c_int32), ("diag_mode", C.c_int32), ("B", C.c_int64), ("N", C.c_int64), ("R", C.c_int64),
                   ("n2", C.c_int64), ("A0", C.c_void_p), ("A1", C.c_void_p), ("d", C.c_void_p),
                   ("nterms", C.c_int32), ("reserved", C.c_int32), ("terms", C.POINTER(OpDesc))]


class InterpDesc(C.Structure):
    """lo_interp_desc (include/lo_amd.h): the interpolation matrices of an LO_OP_SKI_DIAG / LO_OP_SKI_GRID_DIAG
    descriptor, reached through the descriptor's `terms` slot (a union in C); the grid shape of the grid kind (zeros: a
    1-D grid)."""
    _fields_ = [("left_idx", C.c_void_p), ("left_vals", C.c_void_p), ("right_idx", C.c_void_p),
                ("right_vals", C.c_void_p), ("right_plan", C.c_void_p), ("grid_ndim", C.c_int32),
                ("grid_reserved", C.c_int32), ("grid_m", C.c_int64 * 3)]


class GridDesc(C.Structure):
    """lo_grid_desc (include/lo_amd.h): the grid shape of an LO_OP_TOEPLITZ_KRON_DIAG descriptor, reached through the
    descriptor's `terms` slot (a union in C)."""
    _fields_ = [("ndim", C.c_int32), ("reserved", C.c_int32), ("m", C.c_int64 * 3)]


class MaskDesc(C.Structure):
    """lo_mask_desc (include/lo_amd.h): the base descriptor and the selected rows of an LO_OP_MASKED descriptor, reached
    through the descriptor's `terms` slot (a union in C)."""
    _fields_ = [("base", C.POINTER(OpDesc)), ("idx", C.c_void_p), ("M", C.c_int64)]


class PrecondDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("ldq", C.c_int32), ("constant_diag", C.c_int32), ("reserved", C.c_int32),
                ("Q", C.c_void_p), ("dinv", C.c_void_p), ("F", C.c_void_p), ("EF", C.c_void_p), ("E", C.c_void_p),
                ("rf_ld", C.c_int32), ("generation", C.c_int32),
                ("kron_a", C.c_void_p), ("kron_b", C.c_void_p), ("kron_F", C.c_void_p), ("RS", C.c_void_p),
                ("RSD", C.c_void_p)]


class CgParams(C.Structure):
    _fields_ = [("c", C.c_int64), ("n_tridiag", C.c_int32), ("max_iter", C.c_int32), ("max_tridiag_iter", C.c_int32),
                ("floor_max_iter", C.c_int32), ("tolerance", C.c_float), ("eps", C.c_float),
                ("stop_updating_after", C.c_float), ("pad", C.c_float), ("stop_reduce", STOP_REDUCE_CB),
                ("stop_reduce_user", C.c_void_p)]


class CgInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("matvecs", C.c_int32), ("tolerance_reached", C.c_int32),
                ("nan_detected", C.c_int32), ("skipped", C.c_int32), ("last_tridiag_iter", C.c_int32),
                ("mean_residual", C.c_float), ("reserved", C.c_float)]


class CgPlan(C.Structure):
    """lo_cg_plan (include/lo_amd.h): the engine selection of lo_cg_solve_f32."""
    _fields_ = [(n, C.c_int32) for n in (
        "resident", "resident_iterations", "lockstep_cols", "lockstep_group", "serial_engine", "serial_group", "lean",
        "needs_q", "streaming_precond", "poll_chunk", "first_stop_iteration", "streaming_iterations", "rspace",
        "rspace_diag")]


class ResidentStatus(C.Structure):
    """lo_resident_status (include/lo_amd.h): the gate of the resident kernels."""
    _fields_ = [(n, C.c_int32) for n in ("user_disabled", "timeouts", "cooldown", "backoff", "rearms", "fused_timeouts")]


ENGINE_NAMES = {0: "none", 1: "gen1", 2: "gen2", 3: "root"}
STREAM_PRE_NAMES = {0: "none", 1: "two_pass", 2: "closure", 3: "fused_q", 4: "fused_kron", 5: "fused_cols",
                    6: "fused_cols_nopre"}


class FusedInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("matvecs", C.c_int32),
                ("tolerance_reached", C.c_int32), ("nan_detected", C.c_int32), ("skipped", C.c_int32),
                ("rank", C.c_int32), ("mean_residual", C.c_float)]


class CgParamsF64(C.Structure):
    _fields_ = [("c", C.c_int64), ("n_tridiag", C.c_int32), ("max_iter", C.c_int32), ("max_tridiag_iter", C.c_int32),
                ("floor_max_iter", C.c_int32), ("tolerance", C.c_double), ("eps", C.c_double),
                ("stop_updating_after", C.c_double)]


class CgInfoF64(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("matvecs", C.c_int32), ("tolerance_reached", C.c_int32),
                ("nan_detected", C.c_int32), ("skipped", C.c_int32), ("last_tridiag_iter", C.c_int32),
                ("mean_residual", C.c_double)]


class F64OpCtx(C.Structure):
    """lo_f64_op_ctx: the `user` of lo_matvec_desc_cb_f64."""
    _fields_ = [("op", C.POINTER(OpDesc)), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class F64PrecondCtx(C.Structure):
    """lo_f64_precond_ctx: the `user` of lo_precond_desc_cb_f64."""
    _fields_ = [("Q", C.c_void_p), ("noise", C.c_void_p), ("diag_mode", C.c_int32), ("k", C.c_int32),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class MinresParamsF64(C.Structure):
    _fields_ = [("c", C.c_int64), ("n_shifts", C.c_int32), ("max_iter", C.c_int32), ("has_value", C.c_int32),
                ("shifts_per_member", C.c_int32), ("value", C.c_double), ("tolerance", C.c_double), ("eps", C.c_double)]


class MinresInfoF64(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("matvecs", C.c_int32), ("converged", C.c_int32), ("pad", C.c_int32),
                ("conv", C.c_double)]


class MinresParams(C.Structure):
    _fields_ = [("c", C.c_int64), ("n_shifts", C.c_int32), ("max_iter", C.c_int32), ("has_value", C.c_int32),
                ("shifts_per_member", C.c_int32), ("value", C.c_float), ("tolerance", C.c_float), ("eps", C.c_float),
                ("pad", C.c_float)]


class MinresInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("matvecs", C.c_int32), ("converged", C.c_int32), ("conv", C.c_float)]


ROWFETCH_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)
MATVEC_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p)

# The C ABI of include/lo_amd.h, one line per entry point: name -> (restype, argtypes).  load() applies it; pointers to
# device memory and opaque handles (workspaces, streams, callback user data) are void*.
ci, i32, i64, f32, f64, sz, vp, P = C.c_int, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_void_p, C.POINTER
_PROTOTYPES = {
    "lo_abi_version": (ci, []),
    "lo_target_arch": (C.c_char_p, []),
    "lo_matvec_workspace_bytes": (sz, [P(OpDesc), i64]),
    "lo_matvec_f32": (ci, [P(OpDesc), vp, vp, i64, vp, sz, vp]),
    "lo_cg_workspace_bytes": (sz, [P(OpDesc), P(PrecondDesc), P(CgParams)]),
    "lo_cg_solve_f32": (ci, [P(OpDesc), MATVEC_CB, vp, P(PrecondDesc), MATVEC_CB, vp, P(CgParams), vp, vp, vp, vp, vp,
                              sz, P(CgInfo), vp]),
    "lo_cg_session_workspace_bytes": (sz, [P(OpDesc), P(CgParams)]),
    "lo_cg_session_create_f32": (ci, [P(OpDesc), P(PrecondDesc), P(CgParams), vp, sz, P(vp)]),
    "lo_cg_session_solve_f32": (ci, [vp, vp, vp, P(CgInfo), P(CgPlan), vp]),
    "lo_cg_session_destroy": (None, [vp]),
    "lo_cg_session_debug_live": (ci, []),
    "lo_cg_set_onchip": (ci, [ci]),
    "lo_cg_plan_f32": (ci, [P(OpDesc), P(PrecondDesc), ci, ci, P(CgParams), ci, P(CgPlan)]),
    "lo_cg_last_executed": (ci, [P(CgPlan)]),
    "lo_resident_status_get": (ci, [P(ResidentStatus)]),
    "lo_resident_inject_timeouts": (ci, [i32]),
    "lo_resident_handoff_debug": (ci, [i32, i64, i64, P(C.c_uint32)]),
    "lo_resident_order_debug": (ci, [i32, P(C.c_uint32)]),
    "lo_resident_start_debug": (ci, [i32, i32, P(C.c_uint32)]),
    "lo_resident_start_delay": (ci, [i32, i32, i64, i32, i32]),
    "lo_solve_fused_supported": (ci, [P(OpDesc), i32, P(CgParams)]),
    "lo_solve_fused_workspace_bytes": (sz, [P(OpDesc), i32, P(CgParams)]),
    "lo_solve_fused_f32": (ci, [P(OpDesc), i32, f32, P(CgParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, P(FusedInfo),
                                 vp]),
    "lo_solve_fused_perm": (ci, [vp, i64, i64, i32, vp, vp]),
    "lo_cg_f64_workspace_bytes": (sz, [i64, i64, P(CgParamsF64)]),
    "lo_cg_solve_f64": (ci, [vp, vp, MATVEC_CB, vp, MATVEC_CB, vp, P(CgParamsF64), i64, i64, vp, vp, vp, vp, vp, sz,
                              P(CgInfoF64), vp]),
    "lo_minres_f64_workspace_bytes": (sz, [i64, i64, P(MinresParamsF64)]),
    "lo_minres_f64": (ci, [vp, vp, MATVEC_CB, vp, MATVEC_CB, vp, P(MinresParamsF64), i64, i64, vp, vp, vp, vp, sz,
                            P(MinresInfoF64), vp]),
    "lo_matvec_f64_workspace_bytes": (sz, [P(OpDesc), i64]),
    "lo_matvec_f64": (ci, [P(OpDesc), vp, vp, i64, vp, sz, vp]),
    "lo_matvec_desc_cb_f64": (ci, [vp, vp, vp, i64, i64, i64, vp]),
    "lo_precond_f64_workspace_bytes": (sz, [i64, i64, i32, i64]),
    "lo_precond_desc_cb_f64": (ci, [vp, vp, vp, i64, i64, i64, vp]),
    "lo_pivoted_cholesky_workspace_bytes": (sz, [P(OpDesc), i32]),
    "lo_pivoted_cholesky_f32": (ci, [P(OpDesc), i32, f32, vp, vp, P(i32), vp, sz, vp]),
    "lo_pivoted_cholesky_cb_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_pivoted_cholesky_cb_f32": (ci, [i64, i64, vp, ROWFETCH_CB, vp, i32, f32, vp, vp, P(i32), vp, sz, vp]),
    "lo_pivoted_cholesky_f64_workspace_bytes": (sz, [P(OpDesc), i32]),
    "lo_pivoted_cholesky_f64": (ci, [P(OpDesc), i32, f64, vp, vp, P(i32), vp, sz, vp]),
    "lo_pivoted_cholesky_cb_f64_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_pivoted_cholesky_cb_f64": (ci, [i64, i64, vp, ROWFETCH_CB, vp, i32, f64, vp, vp, P(i32), vp, sz, vp]),
    "lo_precond_build_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_precond_build_f32": (ci, [vp, vp, i32, i64, i64, i32, vp, vp, vp, vp, sz, vp]),
    "lo_precond_build_strided_f32": (ci, [vp, i64, i64, i64, vp, i32, i64, i64, i32, vp, vp, vp, vp, sz, vp]),
    "lo_precond_apply_workspace_bytes": (sz, [i64, i64, i32, i64]),
    "lo_precond_apply_f32": (ci, [P(PrecondDesc), vp, vp, i64, i64, i64, vp, sz, vp]),
    "lo_precond_root_form_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_precond_root_form_f32": (ci, [vp, i32, vp, i32, vp, i64, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp,
                                       vp, sz, vp]),
    "lo_precond_root_form_rs_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_precond_root_form_rs_f32": (ci, [vp, i32, vp, i32, vp, i64, i64, i64, vp, i64, i64, i32, i32, vp, vp, vp, vp,
                                          vp, vp, vp, sz, vp]),
    "lo_precond_eigform_f32": (ci, [vp, i64, i32, i32, vp, vp]),
    "lo_precond_kron_root_workspace_bytes": (sz, [i64]),
    "lo_precond_kron_root_f32": (ci, [P(OpDesc), vp, i64, i64, i64, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    "lo_lanczos_workspace_bytes": (sz, [P(OpDesc), i64, i32]),
    "lo_lanczos_tridiag_f32": (ci, [P(OpDesc), MATVEC_CB, vp, vp, i64, i32, f32, vp, vp, P(i32), vp, sz, vp]),
    "lo_lanczos_permute_f32": (ci, [vp, i32, i64, i64, i64, vp, vp]),
    "lo_root_from_lanczos_f32": (ci, [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp]),
    "lo_root_from_lanczos_native_f32": (ci, [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp]),
    "lo_lanczos_f64_workspace_bytes": (sz, [i64, i64, i64, i32]),
    "lo_lanczos_tridiag_f64": (ci, [vp, vp, MATVEC_CB, vp, vp, i64, i64, i64, i32, f64, vp, vp, P(i32), vp, sz, vp]),
    "lo_tridiag_eigh_slq_workspace_bytes": (sz, [i64, i64]),
    "lo_tridiag_eigh_slq_f32": (ci, [vp, i64, i64, i32, i64, vp, vp, vp, vp, sz, vp]),
    "lo_bilinear_dense_f32": (ci, [vp, vp, i64, i64, i64, vp, vp]),
    "lo_bilinear_diag_f32": (ci, [vp, vp, i64, i64, i64, i32, vp, vp, sz, vp]),
    "lo_bilinear_root_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "lo_bilinear_root_f32": (ci, [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, sz, vp]),
    "lo_bilinear_kron_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "lo_bilinear_kron_f32": (ci, [vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, sz, vp]),
    "lo_root_apply_add_f32": (ci, [vp, vp, i64, i64, i64, i64, vp, vp]),
    "lo_minres_workspace_bytes": (sz, [P(OpDesc), P(PrecondDesc), P(MinresParams)]),
    "lo_minres_f32": (ci, [P(OpDesc), MATVEC_CB, vp, P(PrecondDesc), MATVEC_CB, vp, P(MinresParams), vp, vp, vp, vp, sz,
                            P(MinresInfo), vp]),
    "lo_probe_vectors_workspace_bytes": (sz, [i64, i64, i64]),
    "lo_probe_vectors_f32": (ci, [vp, i64, i64, i64, i32, vp, i32, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, sz, vp]),
    "lo_iql_backward_factors_f32": (ci, [vp, vp, i64, vp, vp, vp, f32, i64, i64, i64, i64, vp, vp, vp, vp, vp]),
    "lo_interp_f32": (ci, [vp, vp, i64, i64, i64, i64, vp, i64, vp, vp]),
    "lo_interp_t_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "lo_interp_t_f32": (ci, [vp, vp, i64, i64, i64, i64, vp, i64, vp, vp, sz, vp]),
    "lo_interp_plan_bytes": (sz, [i64, i64, i64, i64]),
    "lo_interp_plan_build": (ci, [vp, i64, i64, i64, i64, vp, sz, vp]),
    "lo_interp_t_planned_f32": (ci, [vp, vp, i64, i64, i64, i64, vp, i64, vp, vp]),
    "lo_interp_sum_f32": (ci, [vp, vp, i64, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, vp]),
    "lo_interp_t_bcast_planned_f32": (ci, [vp, vp, i64, i64, i64, i64, i64, vp, i64, vp, vp]),
    "lo_toeplitz_workspace_bytes": (sz, [i64, i64, i64]),
    "lo_toeplitz_mv_f32": (ci, [vp, i64, i64, vp, i64, vp, vp, sz, vp]),
    "lo_toeplitz_bilinear_f32": (ci, [vp, vp, i64, i64, i64, vp, vp, sz, vp]),
    "lo_interp_values_grad_f32": (ci, [vp, i64, i64, i64, i64, vp, vp, i64, vp, vp]),
    "lo_toeplitz_kron_workspace_bytes": (sz, [P(i64), ci, i64, i64]),
    "lo_toeplitz_kron_mv_f32": (ci, [vp, P(i64), ci, i64, vp, i64, vp, vp, sz, vp]),
    "lo_toeplitz_kron_bilinear_workspace_bytes": (sz, [P(i64), ci, i64, i64]),
    "lo_toeplitz_kron_bilinear_f32": (ci, [vp, P(i64), ci, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kron_eig_apply_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "lo_kron_eig_apply_f32": (ci, [vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, sz, vp]),
    "lo_hadamard_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_hadamard_bilinear_f32": (ci, [vp, vp, vp, vp, i64, i64, i64, i64, i64, vp, vp, vp, sz, vp]),
    "lo_kernel_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_bilinear_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_points_grad_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_points_grad_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_mv_f64_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_mv_f64": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_bilinear_f64_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_bilinear_f64": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_points_grad_f64_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_points_grad_f64": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_sum_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sum_mv_f32": (ci, [vp, vp, vp, P(i32), i64, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_sum_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sum_bilinear_f32": (ci, [vp, vp, vp, P(i32), i64, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_sum_points_grad_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sum_points_grad_f32": (ci, [vp, vp, vp, P(i32), i64, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_kron_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_kron_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_lmc_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_lmc_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_grad_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_grad_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_grad_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_grad_bilinear_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_task_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_task_mv_f32": (ci, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_task_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_task_bilinear_f32": (ci, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, i64, vp, vp, vp, sz, vp]),
    "lo_kernel_task_points_grad_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_task_points_grad_f32": (ci, [vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_param_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_param_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_param_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_param_bilinear_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_param_points_grad_workspace_bytes": (sz, [i64, i64, i64, i64, i64]),
    "lo_kernel_param_points_grad_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_sm_mv_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sm_mv_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, i64, vp, i32, vp, vp, sz, vp]),
    "lo_kernel_sm_bilinear_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sm_bilinear_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_kernel_sm_points_grad_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64]),
    "lo_kernel_sm_points_grad_f32": (ci, [vp, vp, vp, i32, i64, i64, i64, i64, vp, vp, i64, vp, vp, sz, vp]),
    "lo_cholesky_workspace_bytes": (sz, [i64, i64]),
    "lo_cholesky_f32": (ci, [vp, vp, vp, vp, i64, i64, vp, sz, vp]),
    "lo_tri_solve_f32": (ci, [vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]),
    "lo_cholesky_solve_f32": (ci, [vp, vp, vp, i64, i64, i64, i32, vp]),
    "lo_cholesky_f64_workspace_bytes": (sz, [i64, i64]),
    "lo_cholesky_f64": (ci, [vp, vp, vp, vp, i64, i64, vp, sz, vp]),
    "lo_tri_solve_f64": (ci, [vp, vp, vp, vp, i64, i64, i64, i32, i32, vp]),
    "lo_cholesky_solve_f64": (ci, [vp, vp, vp, i64, i64, i64, i32, vp]),
    "lo_eigh_f64_workspace_bytes": (sz, [i64, i64, i32]),
    "lo_eigh_f64": (ci, [vp, vp, vp, vp, i64, i64, i32, vp, sz, vp]),
    "lo_mask_expand_workspace_bytes": (sz, [i64]),
    "lo_mask_expand_f32": (ci, [vp, i64, i64, vp, vp, i64, i64, vp, sz, vp]),
    "lo_block_mv_workspace_bytes": (sz, [P(OpDesc), i32, i64, i64]),
    "lo_block_mv_f32": (ci, [P(OpDesc), i32, i64, vp, vp, i64, vp, sz, vp]),
    "lo_prof_enable": (ci, [ci]),
    "lo_prof_report": (ci, [C.c_char_p, sz]),
    "lo_hbm_triad_f32": (ci, [vp, vp, vp, f32, sz, vp]),
    "lo_hbm_copy_f32": (ci, [vp, vp, sz, vp]),
    "lo_hbm_stream_dev": (ci, [ci, ci, ci, vp, vp, vp, f32, sz, vp]),
    "lo_peer_gather_set": (ci, [P(vp), ci, C.c_longlong]),
}
del ci, i32, i64, f32, f64, sz, vp, P
EXPORTS = list(_PROTOTYPES)


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load liblo_amd.so (after torch, so that both share one HIP runtime).  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise HipExtensionError(
            f"liblo_amd.so not found at {_LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C linear_operator_amd/csrc`). linear_operator_amd has no CPU fallback."
        )
    lib = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    missing = []
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            missing.append(name)
            continue
        fn.restype = restype
        fn.argtypes = argtypes
    if "lo_abi_version" not in missing and lib.lo_abi_version() != ABI_VERSION:
        raise HipExtensionError(f"liblo_amd.so ABI {lib.lo_abi_version()} != binding {ABI_VERSION}; rebuild")
    if missing:
        raise HipExtensionError(f"liblo_amd.so does not export {missing}; rebuild it")
    _lib = lib
    return lib


_FAST_PATH = os.path.join(os.path.dirname(_LIB_PATH), "_lo_pyfast.so")
_fast = False  # False: not tried yet; None: not built or not importable; else the bound module


def _import_fast():
    """The extension module csrc/lo_pyfast.cpp, from the file the csrc Makefile wrote beside liblo_amd.so."""
    from importlib.machinery import ExtensionFileLoader
    from importlib.util import module_from_spec, spec_from_file_location

    spec = spec_from_file_location("_lo_pyfast", _FAST_PATH, loader=ExtensionFileLoader("_lo_pyfast", _FAST_PATH))
    mod = module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fast():
    """_lo_pyfast bound to the entry points of the CDLL load() holds (it is not linked against liblo_amd.so: it calls
    the very image ctypes loaded), or None if it is not built or does not import -- the ctypes binding serves then."""
    global _fast
    if _fast is False:
        lib = load()
        try:
            mod = _import_fast() if os.path.exists(_FAST_PATH) else None
            if mod is not None:
                mod.bind(C.cast(lib.lo_cg_session_solve_f32, C.c_void_p).value)
        except Exception:  # noqa: BLE001 -- optional: another interpreter's build, a truncated file
            mod = None
        _fast = mod
    return _fast


def prof_enable(on):
    """True / 1: HIP-event scopes around the launches; 2: host intervals of the entry points only ("host:<name>" lines of
    prof_report, no events inside them); 3: both; False / 0: off."""
    load().lo_prof_enable(int(on))


def prof_report() -> dict:
    """{kernel_class: (launch_count, total_ms)} since the last report (HIP events on the launch stream)."""
    buf = C.create_string_buffer(1 << 16)
    load().lo_prof_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out


def hbm_stream_gbs(device, mode: str = "triad", n_floats: int = 1 << 28, reps: int = 10, unroll=None, nt=None) -> float:
    """Achievable HBM rate of this box in GB/s: `triad` a = b + s c (12 bytes per element), `copy` a = b (8 bytes),
    `read` (8 bytes), over n-float arrays (1 GiB each by default: far beyond the 256 MiB Infinity Cache).  `unroll` /
    `nt` select a variant of the sweep aid instead of the library's default shape."""
    lib = load()
    a, b, c = (torch.empty(n_floats, dtype=torch.float32, device=device) for _ in range(3))
    b.fill_(1.0)
    c.fill_(2.0)
    st = stream_ptr(device)
    code = {"triad": 0, "copy": 1, "read": 2}[mode]
    nbytes = {"triad": 12, "copy": 8, "read": 8}[mode]

    def launch():
        if unroll is not None:
            return lib.lo_hbm_stream_dev(code, unroll, 1 if nt else 0, ptr(a), ptr(b), ptr(c), 0.5, n_floats, st)
        if mode == "triad":
            return lib.lo_hbm_triad_f32(ptr(a), ptr(b), ptr(c), 0.5, n_floats, st)
        if mode == "copy":
            return lib.lo_hbm_copy_f32(ptr(a), ptr(b), n_floats, st)
        return lib.lo_hbm_stream_dev(2, 4, 1, ptr(a), ptr(b), ptr(c), 0.5, n_floats, st)

    check(launch(), "lo_hbm_stream")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize(device)
    return nbytes * n_floats * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def hbm_triad_gbs(device, n_floats: int = 1 << 28, reps: int = 10) -> float:
    return hbm_stream_gbs(device, "triad", n_floats, reps)


def check(rc: int, what: str):
    if rc != 0:
        raise HipExtensionError(f"liblo_amd {what} failed: {_ERR.get(rc, rc)}")


def call(name: str, *args):
    """Call the entry point `name`; a non-zero return raises through check() under that name.  Entry points whose
    non-zero return is a decision of the library (LO_ERR_UNSUPPORTED: take the other path) are called directly."""
    check(getattr(load(), name)(*args), name)


def require_hip(*tensors: Optional[torch.Tensor], dtype=torch.float32):
    """Every tensor must be a HIP tensor of `dtype` (fp32 everywhere but the fp64 linear_cg entry); anything else is an
    error (no CPU path exists)."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipExtensionError(
                "linear_operator_amd's iterative solvers run only on MI355X device tensors (got a CPU tensor); "
                "there is no CPU fallback -- move the operator / right-hand side to 'cuda'."
            )
        if t.dtype != dtype:
            raise HipExtensionError(
                f"liblo_amd kernels are fp32 (linear_cg on dense tensors / closures also fp64); got {t.dtype} where "
                f"{dtype} was expected")


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (device index) -> the current stream's handle as an int


def stream_ptr(device=None):
    """The current HIP stream of `device` as a raw handle (torch._C._cuda_getCurrentRawStream: 0.3 us instead of the 4 us
    of building a torch.cuda.Stream object -- this sits on every solve's critical path)."""
    raw = RAW_STREAM
    if raw is None:
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    if device is None:
        idx = torch.cuda.current_device()
    else:
        dev = torch.device(device) if not isinstance(device, torch.device) else device
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return C.c_void_p(raw(idx))


def workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class DevArray:
    """Borrowed device pointer exposed through __cuda_array_interface__ so that torch can view it
    (used to hand the C engine's buffers to Python matvec closures without a copy)."""

    def __init__(self, p: int, shape, typestr: str = "<f4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(p), False),
                                         "version": 2, "strides": None}


def as_tensor(p: int, shape, device, typestr: str = "<f4") -> torch.Tensor:
    return torch.as_tensor(DevArray(p, shape, typestr), device=device)
