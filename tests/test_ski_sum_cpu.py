"""Additive SKI (LO_OP_SKI_SUM_DIAG) without a GPU: the ABI pieces, the refusals of the kind (placeholder pointers: every
refusal comes before a launch), and the CPU composition SumBatch(Interpolated(Toeplitz)) of this package against the
reference's goldens tests/golden/g45_ski_sum_*.npz (made by tests/golden/make_golden_ski_sum.py).  The solvers and the
pivoted Cholesky of this package are device code: their goldens are met in tests/test_gpu_ski_sum.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import ski_sum_cases as S  # noqa: E402

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    InterpolatedLinearOperator, SumBatchLinearOperator, ToeplitzLinearOperator)

X = S.ski_sum_inputs()
HDR = open(os.path.join(ROOT, "include", "lo_amd.h")).read()
FAKE = 0x1000  # a non-null pointer that is never dereferenced: the refusals come before any launch
BAD, WS, UNSUP = -1, -3, _hip.LO_ERR_UNSUPPORTED  # LO_ERR_BADARG, LO_ERR_WORKSPACE (include/lo_amd.h)


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or not t.dtype.is_floating_point else t.to(dtype)


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def operator(p, shared=False, dtype=None):
    col, li, lv = T(X[p + "_col"], dtype), T(X[p + "_li"]), T(X[p + "_lv"], dtype)
    ri, rv = (li, lv) if shared else (T(X[p + "_ri"]), T(X[p + "_rv"], dtype))
    return SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, ri, rv))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_constants_abi_and_exports():
    assert _hip.ABI_VERSION >= 37 and _hip.load().lo_abi_version() == _hip.ABI_VERSION
    assert _hip.LO_OP_SKI_SUM_DIAG == 16 and _hip.LO_SKI_SUM_MAX_TERMS == 64
    for name in ("LO_OP_SKI_SUM_DIAG", "LO_SKI_SUM_MAX_TERMS"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", HDR).group(1)) == getattr(_hip, name)
    lib = _hip.load()
    for name in ("lo_interp_sum_f32", "lo_interp_t_bcast_planned_f32"):
        assert re.search(rf"\b{name}\s*\(", HDR), name
        assert name in _hip.EXPORTS and hasattr(lib, name)
    # the two structs keep the size and layout of ABI 36
    assert ctypes.sizeof(_hip.OpDesc) == 80 and _hip.OpDesc.terms.offset == 72 and ctypes.sizeof(_hip.InterpDesc) == 72


# ---- descriptors with placeholder pointers ------------------------------------------------------------------------------
def desc16(B=2, P=3, N=300, M=64, J=4, **over):
    w = _hip.InterpDesc(FAKE, FAKE, FAKE, FAKE, None)
    s = _hip.OpDesc()
    s.kind, s.diag_mode, s.B, s.N, s.R, s.n2, s.A0, s.nterms = _hip.LO_OP_SKI_SUM_DIAG, 0, B, N, M, J, FAKE, P
    s.terms = ctypes.cast(ctypes.pointer(w), ctypes.POINTER(_hip.OpDesc))
    s._keep = w
    for k, v in over.items():
        if k in ("left_idx", "left_vals", "right_idx", "right_vals", "right_plan"):
            setattr(w, k, v)
        elif k == "interp":
            s.terms = None
        else:
            setattr(s, k, v)
    return s


REFUSALS = [
    ("a null A0", dict(A0=None), BAD), ("a null interp", dict(interp=None), BAD),
    ("a null left_idx", dict(left_idx=None), BAD), ("a null left_vals", dict(left_vals=None), BAD),
    ("a null right_idx", dict(right_idx=None), BAD), ("a null right_vals", dict(right_vals=None), BAD),
    ("P = 0", dict(nterms=0), BAD), ("P = -1", dict(nterms=-1), BAD), ("J = 0", dict(n2=0), BAD),
    ("a diagonal mode without d", dict(diag_mode=_hip.LO_DIAG_FULL), BAD),
    ("P above the limit", dict(nterms=_hip.LO_SKI_SUM_MAX_TERMS + 1), UNSUP),
    ("M above the limit", dict(R=_hip.LO_TOEPLITZ_MAX_M + 1), UNSUP),
    ("N J beyond 32 bits", dict(N=1 << 29, n2=4), UNSUP),
]


def matvec_rc(s, c=1, ws_bytes=1 << 40):
    return _hip.load().lo_matvec_f32(ctypes.byref(s), FAKE, FAKE, c, FAKE, ws_bytes, None)


def test_workspace_query_is_positive_and_grows_with_the_terms():
    lib = _hip.load()
    need = [lib.lo_matvec_workspace_bytes(ctypes.byref(desc16(P=P)), 3) for P in (1, 3)]
    assert 0 < need[0] < need[1]
    # u and T u [B, P, M, c] alone
    assert need[1] >= 2 * 2 * 3 * 64 * 3 * 4
    # P = 1: the layout of LO_OP_SKI_DIAG
    ski = desc16(P=1)
    ski.kind, ski.nterms = _hip.LO_OP_SKI_DIAG, 0
    assert need[0] == lib.lo_matvec_workspace_bytes(ctypes.byref(ski), 3)
    # a kept right_plan: the copy of W_r leaves the workspace
    kept = lib.lo_matvec_workspace_bytes(ctypes.byref(desc16(right_plan=FAKE)), 3)
    assert kept + lib.lo_interp_plan_bytes(2 * 3, 300, 4, 64) - 256 <= need[1] and kept < need[1]


@pytest.mark.parametrize("what,over,rc", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_product_and_the_pivoted_cholesky(what, over, rc):
    lib = _hip.load()
    assert matvec_rc(desc16(**over)) == rc, what
    if "diag_mode" in over:  # (the pivoted Cholesky factors the operator without its diagonal)
        return
    rank = ctypes.c_int32(0)
    s = desc16(**over)
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), 10, 1e-3, FAKE, FAKE, ctypes.byref(rank), FAKE, 1 << 40,
                                       None) == rc, what


def test_short_workspace_is_refused_before_the_plan_is_built():
    s = desc16()
    need = _hip.load().lo_matvec_workspace_bytes(ctypes.byref(s), 3)
    assert matvec_rc(s, 3, need - 1) == WS
    assert _hip.load().lo_matvec_f32(ctypes.byref(s), FAKE, FAKE, 3, None, need, None) == WS


def test_entry_points_that_do_not_lower_the_kind():
    lib = _hip.load()
    s = desc16()
    for fn in (lib.lo_matvec_f64,):
        assert fn(ctypes.byref(s), FAKE, FAKE + 64, 1, FAKE, 1 << 40, None) == UNSUP
    rank = ctypes.c_int32(0)
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 10, 1e-3, FAKE, FAKE, ctypes.byref(rank), FAKE, 1 << 40,
                                       None) == UNSUP
    prm = _hip.CgParams()
    prm.c, prm.max_iter, prm.max_tridiag_iter, prm.tolerance, prm.eps, prm.stop_updating_after = 1, 100, 20, 1e-4, 1e-10, 1e-10
    s.diag_mode, s.d = _hip.LO_DIAG_FULL, FAKE
    assert lib.lo_solve_fused_supported(ctypes.byref(s), 15, ctypes.byref(prm)) == 0
    s = desc16()
    assert lib.lo_block_mv_f32(ctypes.byref(s), _hip.LO_BLOCK_SUM, 2, FAKE, FAKE, 1, FAKE, 1 << 40, None) == UNSUP
    # a term of LO_OP_SUM: not a plain term kind
    root = _hip.OpDesc()
    root.kind, root.B, root.N, root.R, root.A0 = _hip.LO_OP_LOWRANK_DIAG, 2, 300, 8, FAKE
    terms = (_hip.OpDesc * 2)(root, desc16())
    tot = _hip.OpDesc()
    tot.kind, tot.B, tot.N, tot.nterms = _hip.LO_OP_SUM, 2, 300, 2
    tot.terms = ctypes.cast(terms, ctypes.POINTER(_hip.OpDesc))
    assert matvec_rc(tot) == BAD
    # the base of LO_OP_MASKED
    base = desc16()
    m = _hip.MaskDesc(ctypes.pointer(base), FAKE, 8)
    msk = _hip.OpDesc()
    msk.kind, msk.B, msk.N = _hip.LO_OP_MASKED, 2, 8
    msk.terms = ctypes.cast(ctypes.pointer(m), ctypes.POINTER(_hip.OpDesc))
    assert matvec_rc(msk) == UNSUP


def test_building_block_refusals():
    lib = _hip.load()
    ok = dict(B=2, P=3, N=30, J=4, M=16)

    def isum(idx=FAKE, vals=FAKE, u=FAKE, d=None, mode=0, v=None, y=FAKE, c=2, **k):
        a = {**ok, **k}
        return lib.lo_interp_sum_f32(idx, vals, a["B"], a["P"], a["N"], a["J"], a["M"], u, c, d, mode, v, y, None)

    def bcast(plan=FAKE, vals=FAKE, v=FAKE, out=FAKE, c=2, **k):
        a = {**ok, **k}
        return lib.lo_interp_t_bcast_planned_f32(plan, vals, a["B"], a["P"], a["N"], a["J"], a["M"], v, c, out, None)

    for k in ("idx", "vals", "u", "y"):
        assert isum(**{k: None}) == BAD, k
    assert isum(P=0) == BAD and isum(J=0) == BAD and isum(c=0) == BAD and isum(mode=7, d=FAKE, v=FAKE) == BAD
    assert isum(mode=_hip.LO_DIAG_FULL) == BAD and isum(mode=_hip.LO_DIAG_CONST, d=FAKE) == BAD
    assert isum(P=_hip.LO_SKI_SUM_MAX_TERMS + 1) == UNSUP
    for k in ("plan", "vals", "v", "out"):
        assert bcast(**{k: None}) == BAD, k
    assert bcast(P=0) == BAD and bcast(J=0) == BAD and bcast(P=_hip.LO_SKI_SUM_MAX_TERMS + 1) == UNSUP


# ---- the operator on the CPU ---------------------------------------------------------------------------------------------
def test_sum_of_the_batch_dimension_is_the_class_and_has_no_descriptor_off_the_device():
    A = operator("a")
    assert isinstance(A.base_linear_op.sum(-3), SumBatchLinearOperator)
    assert A._kernel_descriptor() is None  # CPU tensors
    assert operator("a", dtype=torch.float64)._kernel_descriptor() is None


@pytest.mark.parametrize("p", ["a", "b"])
def test_composition_meets_the_goldens(p):
    g = golden("g45_ski_sum_" + p)
    A = operator(p)
    B, P, N, M, J = S.SHAPES[p]
    assert A.shape == (B, N, N)
    for c in S.COLS:
        assert np.allclose(A.matmul(T(X[f"{p}_rhs{c}"])).numpy(), g[f"matmul{c}"], rtol=1e-4, atol=1e-5), c
    rows = S.dense_rows(N)
    dense = A.to_dense().numpy()
    assert np.allclose(dense[:, rows], g["dense_rows"], rtol=1e-4, atol=1e-5)
    assert np.allclose(A._diagonal().numpy(), g["diag"], rtol=1e-4, atol=1e-5)
    # the fixture against the float64 truth of the sparse form: pins the [B, P, ..] layout of the input builders
    ref = S.dense64(*(X[f"{p}_{k}"] for k in ("col", "li", "lv", "ri", "rv")))
    assert np.abs(g["dense_rows"] - ref[:, rows]).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("p", ["a", "b"])
def test_exact_diagonal_of_the_pivoted_cholesky_fixture(p):
    """The pivot search of the reference runs on SumBatch._diagonal(), the exact diagonal (the factor itself is a device
    computation: tests/test_gpu_ski_sum.py)."""
    g = golden("g45_ski_sum_pivchol_" + p)
    A = operator("p" + p, shared=True)
    assert np.allclose(A._diagonal().numpy(), g["diag"], rtol=1e-4, atol=1e-5)
    assert np.allclose(A._approx_diagonal().numpy(), g["diag"], rtol=1e-4, atol=1e-5)
    col, li, lv = X[f"p{p}_col"], X[f"p{p}_li"], X[f"p{p}_lv"]
    ref = np.diagonal(S.dense64(col, li, lv, li, lv), axis1=-2, axis2=-1)
    assert np.abs(g["diag"] - ref).max() <= 1e-5 * np.abs(ref).max()
