"""Float64 structured operators (ABI 22) without a GPU: the binding names the new entry points, the descriptor builders
keep float64 behind an explicit `dtype=`, and the golden g34 (the REAL reference's float64 CG / MINRES / Lanczos on a
low-rank, a Kronecker and a sum operator, tests/golden/make_golden_f64.py) agrees with the numpy oracle at the project's
float64 bars -- 1e-9 relative on solutions, 1e-7 on tridiagonals (tests/test_gpu_fp64.py) -- before any kernel is
involved."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from make_golden_f64 import CASES, CG, LANCZOS_STEPS, MINRES_SHIFTS, MINRES_TOL, f64_inputs
from oracle import lo_oracle as orc

from linear_operator_amd import _hip, kernels as K


def oracle_matvec(case, t):
    if case == "lowrank":
        return lambda v: orc.matvec_lowrank_diag(t["C"], t["d"], v)
    if case == "kron":
        n = t["K1"].shape[-1] * t["K2"].shape[-1]
        d = np.broadcast_to(t["sigma2"], t["sigma2"].shape[:-1] + (n,))
        return lambda v: orc.matvec_kron_diag(t["K1"], t["K2"], d, v)
    return lambda v: (orc.matvec_lowrank_diag(t["C"], np.zeros_like(t["d"]), v) + t["K"] @ v) + t["d"][..., None] * v


def oracle_precond(g, case):
    """precondition_closure (added_diag_linear_operator.py:135-140 of the reference) from the cached pair in g34."""
    Q, noise = g[f"Q_{case}"], g[f"noise_{case}"][..., None]
    if bool(g[f"constant_{case}"]):
        return lambda r: (r - Q @ (np.swapaxes(Q, -1, -2) @ r)) / noise
    return lambda r: r / noise - Q @ (np.swapaxes(Q, -1, -2) @ r)


def test_the_binding_names_the_float64_entry_points_at_abi_22():
    assert _hip.ABI_VERSION >= 22
    for name in ("lo_matvec_f64_workspace_bytes", "lo_matvec_f64", "lo_matvec_desc_cb_f64", "lo_precond_desc_cb_f64",
                 "lo_precond_f64_workspace_bytes"):
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS, name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lo_amd.h")).read()
    for name in ("lo_matvec_f64", "lo_matvec_desc_cb_f64", "lo_precond_desc_cb_f64", "lo_precond_f64_workspace_bytes"):
        assert name + "(" in hdr, name
    assert K.OperatorDescriptor(_hip.LO_OP_DENSE_DIAG, 1, 1).dtype == torch.float32


def test_builders_take_doubles_only_on_request_and_never_mixed():
    C64, C32 = torch.randn(2, 9, 3, dtype=torch.float64), torch.randn(2, 9, 3)
    d64, d32 = torch.rand(2, 9, dtype=torch.float64), torch.rand(2, 9)
    K64, K32 = torch.randn(2, 3, 3, dtype=torch.float64), torch.randn(2, 3, 3)
    mixed = [lambda: K.lowrank_diag_descriptor(C64, d32, dtype=torch.float64),
             lambda: K.lowrank_diag_descriptor(C32, d64, dtype=torch.float64),
             lambda: K.dense_diag_descriptor(K32, None, dtype=torch.float64),
             lambda: K.kron_diag_descriptor(K64, K32, None, dtype=torch.float64),
             lambda: K.kron_diag_descriptor(K64, K64, d32, dtype=torch.float64)]
    for build in mixed:
        with pytest.raises(_hip.HipExtensionError, match="float64 tensors only"):
            build()
    # the default keeps refusing doubles (here on CPU tensors, through the builders' existing check)
    for build in (lambda: K.lowrank_diag_descriptor(C64, None), lambda: K.dense_diag_descriptor(K64, None),
                  lambda: K.kron_diag_descriptor(K64, K64, None)):
        with pytest.raises(_hip.HipExtensionError):
            build()
    with pytest.raises(ValueError):
        K.dense_diag_descriptor(K64, None, dtype=torch.float16)
    # sums: the terms and the sum share one element type
    t32 = K.OperatorDescriptor(_hip.LO_OP_DENSE_DIAG, 2, 9)
    t64 = K.OperatorDescriptor(_hip.LO_OP_DENSE_DIAG, 2, 9, dtype=torch.float64)
    with pytest.raises(_hip.HipExtensionError):
        K.sum_descriptor((t32, t64), dtype=torch.float64)
    with pytest.raises(_hip.HipExtensionError):
        K.sum_descriptor((t64, t64))
    assert K.sum_descriptor((t64, t64), dtype=torch.float64).dtype == torch.float64
    # a float64 descriptor never becomes the C struct of an fp32 entry point, and a diagonal of the other type is refused
    with pytest.raises(_hip.HipExtensionError, match="float64"):
        t64.c_struct()
    with pytest.raises(_hip.HipExtensionError):
        K._with_diag(t64, d32, False)
    assert t64.c_struct(torch.float64).kind == _hip.LO_OP_DENSE_DIAG
    assert t64.without_diag().dtype == torch.float64


@pytest.mark.parametrize("case", CASES)
def test_the_oracle_reproduces_the_reference_float64_cg_of_g34(case):
    g = load_golden("g34_fp64_structured")
    t = f64_inputs(case)
    x, tm, info = orc.linear_cg(oracle_matvec(case, t), t["rhs"], preconditioner=oracle_precond(g, case), **CG)
    assert info.matvecs == int(g[f"matvecs_{case}"]) and info.iterations == info.matvecs - 1
    assert rel_err(x, g[f"x_{case}"]) < 1e-9
    assert tm.shape == g[f"t_{case}"].shape and rel_err(tm, g[f"t_{case}"]) < 1e-7


def test_the_oracle_reproduces_the_reference_float64_minres_and_lanczos_of_g34():
    g = load_golden("g34_fp64_structured")
    t = f64_inputs("kron")
    x, _ = orc.minres(oracle_matvec("kron", t), t["rhs"], shifts=MINRES_SHIFTS, tolerance=MINRES_TOL)
    assert x.shape == g["x_minres"].shape and rel_err(x, g["x_minres"]) < 1e-9
    t = f64_inputs("lowrank")
    q, tl = orc.lanczos_tridiag(oracle_matvec("lowrank", t), LANCZOS_STEPS, t["init"])
    assert tl.shape == g["lanczos_t"].shape
    assert np.allclose(tl, g["lanczos_t"], rtol=1e-9, atol=1e-12)  # (the bars of g26 in tests/test_gpu_fp64.py)
    assert np.allclose(q[0], g["lanczos_q0"], atol=1e-9)
