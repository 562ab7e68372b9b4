"""lo_kernel_param_mv_wide_f32 and lo_kernel_sm_mv_wide_f32 (csrc/lo_kernel_kinds_wide.hip: the kernel value on the vector
ALU as in the one-column kernels, its product with V on v_mfma_f32_32x32x2_f32) on the MI355X against the float64 dense
composition, under the bound of tests/test_gpu_kernel_param.py and test_gpu_kernel_sm.py (their `within`: at most 4 times
the error of the torch float32 composition on the same inputs, floored at ERR_FLOOR); every case prints its ratio."""
import numpy as np
import pytest
import torch

import test_gpu_kernel_param as P
import test_gpu_kernel_sm as S

from linear_operator_amd import _hip, covariance, settings
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

pytestmark = pytest.mark.gpu

DEV, dev, host, rel = P.DEV, P.dev, P.host, P.rel

# M: a 32-row tile, a wave's two tiles, the workgroup edge; N: an odd last MFMA step, the 128-point tile edge, js > 1
# (N > 128); c: a ragged last sweep of 32; B = 512: no column split; a diagonal only on square products.
# (family, B, M, N, D, c, diagonal, ARD, span): both families meet every padded dimension
PARAM_CASES = [
    ("rq", 1, 1, 1, 1, 1, "full", False, 3.0), ("rq", 3, 31, 127, 3, 5, "none", True, 3.0),
    ("rq", 1, 257, 257, 5, 17, "const", True, 3.0), ("rq", 1, 65, 129, 17, 32, "none", False, 3.0),
    ("rq", 1, 33, 3, 32, 33, "none", True, 3.0), ("rq", 1, 129, 129, 1, 65, "full", True, 3.0),
    ("rq", 1, 257, 2, 3, 1, "none", False, 3.0), ("rq", 3, 33, 257, 5, 5, "none", True, 3.0),
    ("rq", 1, 1, 127, 17, 17, "none", False, 3.0), ("rq", 1, 127, 127, 32, 32, "const", True, 3.0),
    ("rq", 3, 130, 77, 3, 17, "none", True, 3.0), ("rq", 512, 33, 129, 3, 17, "none", True, 3.0),
    ("periodic", 1, 65, 1, 1, 33, "none", True, 3.0), ("periodic", 1, 3, 3, 3, 65, "const", False, 3.0),
    ("periodic", 1, 31, 129, 5, 1, "none", True, 3.0), ("periodic", 3, 257, 257, 17, 5, "full", False, 3.0),
    ("periodic", 1, 33, 2, 32, 17, "none", True, 3.0), ("periodic", 1, 257, 127, 1, 32, "none", False, 3.0),
    ("periodic", 1, 2, 2, 3, 33, "full", True, 3.0), ("periodic", 1, 65, 257, 5, 65, "none", False, 3.0),
    ("periodic", 3, 31, 3, 17, 1, "none", True, 3.0), ("periodic", 1, 257, 257, 32, 5, "const", False, 3.0),
    ("periodic", 1, 77, 130, 3, 33, "none", False, 3.0), ("periodic", 2, 257, 257, 2, 17, "full", True, 800.0),
]
# (B, M, N, D, Q, c, diagonal, span): D 1 / 3 / 5 / 16 and Q 1 / 3 / 16
SM_CASES = [
    (1, 1, 1, 1, 1, 1, "full", 3.0), (3, 31, 127, 3, 3, 5, "none", 3.0), (1, 257, 257, 5, 16, 17, "const", 3.0),
    (1, 65, 129, 16, 1, 32, "none", 3.0), (1, 33, 3, 16, 16, 33, "none", 3.0), (1, 129, 129, 1, 3, 65, "full", 3.0),
    (1, 257, 2, 3, 1, 1, "none", 3.0), (3, 33, 257, 5, 3, 5, "none", 3.0), (1, 1, 127, 16, 3, 17, "none", 3.0),
    (1, 127, 127, 1, 16, 32, "const", 3.0), (3, 130, 77, 3, 3, 17, "none", 3.0), (512, 33, 129, 3, 1, 17, "none", 3.0),
    (1, 77, 130, 5, 3, 33, "none", 3.0), (1, 65, 1, 1, 1, 33, "none", 3.0), (1, 3, 3, 3, 16, 65, "const", 3.0),
    (1, 31, 129, 5, 1, 1, "none", 3.0), (3, 257, 257, 16, 3, 5, "full", 3.0), (1, 257, 127, 1, 3, 32, "none", 3.0),
    (1, 2, 2, 3, 3, 33, "full", 3.0), (2, 257, 257, 2, 3, 17, "full", 2400.0),
]


def label(case):
    return "-".join(str(x) for x in case)


@pytest.mark.parametrize("case", PARAM_CASES, ids=label)
def test_param_wide_product_against_the_fp64_composition(case):
    family, B, M, N, D, c, diag, ard, span = case
    x1, x2, ls, os_, sh, v, d = P.make_inputs(9800 + PARAM_CASES.index(case), family, B, M, N, D, c, ard, span)
    if span > 600:
        assert ((x1.max(1) - x1.min(1)) / sh[:, 0]).min() > 600
    if B == 512:
        assert _hip.load().lo_kernel_param_mv_wide_workspace_bytes(B, M, N, D, c) == 256  # (nothing but the tail)
    want = host(P.composition(family, x1, x2, ls, os_, sh, v, d, diag, torch.float64))
    comp = host(P.composition(family, x1, x2, ls, os_, sh, v, d, diag, torch.float32))
    tx1 = dev(x1)
    args = (tx1, tx1 if x2 is x1 else dev(x2), P.theta_of(family, ls, os_, sh, D),
            covariance.PARAM_FAMILIES[family].native_family, dev(v), S.diag_operand(d, diag))
    y = K.kernel_param_mv_wide(*args, const_diag=diag == "const")
    assert y.shape == (B, M, c) and torch.isfinite(y).all()
    P.within("mv_wide " + label(case), rel(host(y), want), rel(comp, want))
    assert torch.equal(K.kernel_param_mv_wide(*args, const_diag=diag == "const"), y)  # two calls give equal bits


@pytest.mark.parametrize("case", SM_CASES, ids=label)
def test_sm_wide_product_against_the_fp64_composition(case):
    B, M, N, D, Q, c, diag, span = case
    x1, x2, w, mu, sg, v, d = S.make_inputs(9900 + SM_CASES.index(case), B, M, N, D, Q, c, span)
    if span > 600:
        assert ((x1.max(1) - x1.min(1))[:, None, :] * mu).max((1, 2)).min() > 600
    if B == 512:
        assert _hip.load().lo_kernel_sm_mv_wide_workspace_bytes(B, M, N, D, Q, c) == 256  # (nothing but the tail)
    want = host(S.composition(x1, x2, w, mu, sg, v, d, diag, torch.float64))
    comp = host(S.composition(x1, x2, w, mu, sg, v, d, diag, torch.float32))
    tx1 = dev(x1)
    args = (tx1, tx1 if x2 is x1 else dev(x2), S.theta_of(w, mu, sg), dev(v), S.diag_operand(d, diag))
    y = K.kernel_sm_mv_wide(*args, const_diag=diag == "const")
    assert y.shape == (B, M, c) and torch.isfinite(y).all()
    S.within("mv_wide " + label(case), rel(host(y), want), rel(comp, want))
    assert torch.equal(K.kernel_sm_mv_wide(*args, const_diag=diag == "const"), y)  # two calls give equal bits


@pytest.mark.parametrize("kind", ["param", "sm"])
def test_wide_entry_points_return_the_error_codes_of_their_twins(kind):
    lib, p = _hip.load(), _hip.ptr
    B, M, D, c, sm = 1, 300, 3, 17, kind == "sm"
    x, v, y = torch.rand(B, M, D, device=DEV), torch.randn(B, M, c, device=DEV), torch.full((B, M, c), -7.0, device=DEV)
    theta = torch.ones(B, 2 * (2 * D + 1) if sm else 2 * D + 2, device=DEV)
    st = _hip.stream_ptr(v.device)
    wide, plain, sizer = ((lib.lo_kernel_sm_mv_wide_f32, lib.lo_kernel_sm_mv_f32, lib.lo_kernel_sm_mv_wide_workspace_bytes)
                          if sm else (lib.lo_kernel_param_mv_wide_f32, lib.lo_kernel_param_mv_f32,
                                      lib.lo_kernel_param_mv_wide_workspace_bytes))
    need = sizer(B, M, M, D, 2, c) if sm else sizer(B, M, M, D, c)  # (> 256: a split member, partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def both(x1=x, second=2 if sm else _hip.LO_KERNEL_RQ, dim=D, mode=0, w=ws, wb=need):  # second: Q or the family
        a = (p(x1), p(x), p(theta), second, B, M, M, dim, p(v), c, None, mode, p(y), p(w), wb, st)
        codes = wide(*a), plain(*a)
        assert codes[0] == codes[1], codes
        return codes[0]

    assert need > 256 and both(x1=None) == -1 and both(mode=1) == -1  # a null pointer, a diagonal mode without d
    assert both(dim=17 if sm else 33) == _hip.LO_ERR_UNSUPPORTED
    assert both(second=17 if sm else 3) == (_hip.LO_ERR_UNSUPPORTED if sm else -1)  # (Q = 17; a family of the plain kind)
    assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: y keeps its fill
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and both() == 0


def solve_17(G, t, op, dense64):
    """(error, the reference's recorded float32 solve error) of a preconditioned solve with 17 right-hand sides on a golden
    case's tensors, against float64 on the stored matrix."""
    rhs = torch.cat((t["rhs"], dev(P.rng(9990).standard_normal((*t["rhs"].shape[:-1], 16)).astype(np.float32))), -1)
    sol = AddedDiagLinearOperator(op, DiagLinearOperator(t["noise"])).solve(rhs)
    want = torch.linalg.solve(dense64 + torch.diag_embed(t["noise"].double()), rhs.double())
    return rel(host(sol), host(want)), max(float(G["solve_err"]), P.ERR_FLOOR)


@pytest.mark.parametrize("family", ["rq", "periodic"])
def test_the_param_kind_takes_the_wide_kernel_where_the_rule_says_so(family):
    """c = 17 at D = 3 is a cell kp_wide (csrc/lo_kernel_shape.h) routes, for both families."""
    B, n, D, c = 3, 300, 3, 17
    x1, _, ls, os_, sh, v, d = P.make_inputs(9980, family, B, n, n, D, c)
    tx, tv, td = dev(x1), dev(v), dev(d)
    fn = covariance.PARAM_FAMILIES[family]
    op = KernelLinearOperator(tx, tx, P.guarded(fn, n), num_nonbatch_dimensions=P.NB, lengthscale=dev(ls),
                              outputscale=dev(os_), **{P.SHAPE[family]: dev(sh)})
    args = (tx, tx, P.theta_of(family, ls, os_, sh, D), fn.native_family, tv)
    want = K.kernel_param_mv_wide(*args)
    assert torch.equal(op._matmul(tv), want)
    assert torch.equal(AddedDiagLinearOperator(op, DiagLinearOperator(td))._matmul(tv), K.kernel_param_mv_wide(*args, td))
    assert torch.equal(K.matvec(K.kernel_param_diag_descriptor(tx, args[2], fn.native_family), tv), want)
    G, t = P.golden(family), P.tensors(family)
    names = ("x", "x", "lengthscale", "outputscale", P.SHAPE[family])
    with P.solver_settings(settings):
        err, ref_err = solve_17(G, t, P.param_op(family, t), fn(*(t[k].double() for k in names)))
    print(f"kernel_param {family} solve, 17 columns: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= P.REF_FACTOR * ref_err


def test_the_sm_kind_takes_the_wide_kernel_where_the_rule_says_so():
    """c = 17 at D = 3 is a cell ksm_wide (csrc/lo_kernel_shape.h) routes."""
    B, n, D, Q, c = 3, 300, 3, 2, 17
    x1, _, w, mu, sg, v, _ = S.make_inputs(9981, B, n, n, D, Q, c)
    tx, tv, theta = dev(x1), dev(v), S.theta_of(w, mu, sg)
    op = KernelLinearOperator(tx, tx, S.guarded(n), num_nonbatch_dimensions=S.NB, mixture_weights=dev(w),
                              mixture_means=dev(mu), mixture_scales=dev(sg))
    want = K.kernel_sm_mv_wide(tx, tx, theta, tv)
    assert torch.equal(op._matmul(tv), want)
    assert torch.equal(K.matvec(K.kernel_sm_diag_descriptor(tx, theta), tv), want)
    G, t = S.golden("ard"), S.tensors("ard")
    with S.solver_settings(settings):
        err, ref_err = solve_17(G, t, S.sm_op("ard", t), S.FN(*(t[k].double() for k in ("x", "x") + S.PARAMS)))
    print(f"kernel_sm ard solve, 17 columns: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= S.REF_FACTOR * ref_err
