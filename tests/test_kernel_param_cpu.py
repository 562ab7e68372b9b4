"""The rational-quadratic and periodic kernels without a GPU: covariance.rq / covariance.periodic against independent
float64 closed forms, the derivative formulas of csrc/lo_kernel_param.hip against float64 autograd,
rq -> rbf for large alpha, the binding of ABI 39 (symbols, constants, the host-side sizers), every branch of the gate
`_native_param_refusal` decided on CPU tensors through its `check_device=False` form (with the other gates answering what
they always did), and the dense path on the CPU against the goldens."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_param import CASES, NB, SHAPE, grad_names, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, SumLinearOperator)

F8 = torch.float64


def rand(g, *shape, lo=0.5, hi=1.5, dtype=F8):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=dtype)


def param_op(x, fn=covariance.rq, x2=None, dtype=torch.float32, ls=None, nb=NB, drop=(), **extra):
    D = x.shape[-1]
    params = {"lengthscale": torch.linspace(0.5, 0.9, max(D, 1), dtype=dtype).reshape(1, max(D, 1)) if ls is None else ls,
              "outputscale": torch.tensor(1.1, dtype=dtype)}
    if fn.native_family == _hip.LO_KERNEL_RQ:
        params["alpha"] = torch.tensor(1.7, dtype=dtype)
    else:
        params["period_length"] = torch.full((1, max(D, 1)), 0.8, dtype=dtype)
    params.update(extra)
    for k in drop:
        del params[k]
    return KernelLinearOperator(x, x if x2 is None else x2, fn, num_nonbatch_dimensions=nb, **params)


@pytest.mark.parametrize("shared", [False, True])
def test_rq_and_periodic_are_the_double_loops(shared):
    """Entry by entry in float64 (math.*, not torch), rectangular and batched, ARD and shared parameters."""
    g = torch.Generator().manual_seed(47)
    n, m, D = 5, 4, 3
    x1, x2 = 3.0 * torch.rand(2, n, D, generator=g, dtype=F8), 3.0 * torch.rand(2, m, D, generator=g, dtype=F8)
    ls, per = rand(g, 2, 1, 1 if shared else D), rand(g, 2, 1, 1 if shared else D, lo=0.6, hi=1.1)
    os_, al = rand(g, 2), rand(g, 2, lo=0.5, hi=3.0)
    got_rq, got_per = covariance.rq(x1, x2, ls, os_, al), covariance.periodic(x1, x2, ls, os_, per)
    assert got_rq.shape == got_per.shape == (2, n, m) and got_rq.dtype == got_per.dtype == F8
    for b in range(2):
        for i in range(n):
            for j in range(m):
                pick = lambda t, k: float(t[b, 0, 0 if shared else k])  # noqa: E731
                r2 = sum(((float(x1[b, i, k]) - float(x2[b, j, k])) / pick(ls, k)) ** 2 for k in range(D))
                want = float(os_[b]) ** 2 * (1.0 + r2 / (2.0 * float(al[b]))) ** (-float(al[b]))
                assert abs(float(got_rq[b, i, j]) - want) <= 1e-14 * max(1.0, abs(want)), (b, i, j)
                rho = sum((math.sin(math.pi * (float(x1[b, i, k]) - float(x2[b, j, k])) / pick(per, k)) / pick(ls, k)) ** 2
                          for k in range(D))
                want = float(os_[b]) ** 2 * math.exp(-2.0 * rho)
                assert abs(float(got_per[b, i, j]) - want) <= 1e-13 * max(1.0, abs(want)), (b, i, j)
    assert covariance.rq(x1.float(), x2.float(), ls.float(), os_.float(), al.float()).dtype == torch.float32
    # the call pattern of `_diagonal` / `_get_indices`: the pairs as a leading batch dimension
    a = x1.movedim(-2, 0).unsqueeze(-2)
    for fn, sh in ((covariance.rq, al), (covariance.periodic, per)):
        blocks = fn(a, a, ls.unsqueeze(0), os_.unsqueeze(0), sh.unsqueeze(0))
        assert torch.allclose(blocks[..., 0, 0].movedim(0, -1), os_.square()[:, None].expand(2, n), rtol=1e-14)


def test_rq_with_a_large_alpha_approaches_rbf():
    g = torch.Generator().manual_seed(48)
    x, ls, os_ = torch.rand(2, 9, 3, generator=g, dtype=F8), rand(g, 2, 1, 3), rand(g, 2)
    want = covariance.rbf(x, x, ls, os_)
    errs = [float((covariance.rq(x, x, ls, os_, torch.full((2,), a, dtype=F8)) - want).abs().max()) for a in (1e2, 1e4, 1e6)]
    assert errs[0] > errs[1] > errs[2] and errs[2] < 1e-5  # (the difference is O(r^4 / alpha))


def theta_leaf(ls, os_, al, per, B, D):
    inv = lambda t: (1.0 / t).expand(B, 1, D)[:, 0]  # noqa: E731
    return torch.cat((inv(ls), os_.square()[:, None], al[:, None], inv(per)), -1).requires_grad_(True)


@pytest.mark.parametrize("family", ["rq", "periodic"])
def test_derivative_formulas_against_fp64_autograd(family):
    """The per-pair formulas the kernels accumulate (g, h, dg/dalpha with its series; the periodic theta, nu and x1 terms),
    summed with weights W in float64, against autograd of the dense function by theta = (1 / l, os^2, alpha, 1 / p)."""
    g = torch.Generator().manual_seed(49)
    B, M, N, D = 2, 7, 6, 3
    x1 = (4.0 * torch.rand(B, M, D, generator=g, dtype=F8)).requires_grad_(True)
    x2 = 4.0 * torch.rand(B, N, D, generator=g, dtype=F8)
    x2[:, 0] = x1[:, 0].detach() + 1e-3  # (a near pair: q below the series threshold)
    ls, per, os_, al = rand(g, B, 1, D), rand(g, B, 1, D, lo=0.7, hi=1.2), rand(g, B), rand(g, B, lo=0.5, hi=3.0)
    W = torch.randn(B, M, N, generator=g, dtype=F8)
    th = theta_leaf(ls, os_, al, per, B, D)
    t, os2, alpha, nu = th[:, :D], th[:, D], th[:, D + 1], th[:, D + 2:]
    fn = covariance.PARAM_FAMILIES[family]
    dense = fn(x1, x2, (1.0 / t)[:, None, :], os2.sqrt(), alpha if family == "rq" else (1.0 / nu)[:, None, :])
    (W * dense).sum().backward()
    with torch.no_grad():
        tk, nk, o2 = t[:, None, None, :], nu[:, None, None, :], os2[:, None, None]
        if family == "rq":
            s = tk * x1[:, :, None, :] - tk * x2[:, None, :, :]
            q = s.square().sum(-1) / (2.0 * alpha[:, None, None])
            gg = (1.0 + q) ** (-alpha[:, None, None])
            h = -gg / (1.0 + q)
            series = -q ** 2 / 2 + 2 * q ** 3 / 3 - 3 * q ** 4 / 4
            small = q < 0.03125
            assert bool(small.any()) and bool((~small).any())
            exact = q / (1.0 + q) - torch.log1p(q)
            assert float(((series - exact).abs() / exact.abs().clamp_min(1e-300))[small].max()) < 5e-5
            ga = gg * torch.where(small, series, exact)
            g_t = (o2 * W * h)[..., None] * s.square() / tk
            want = torch.cat((g_t.sum((1, 2)), (W * gg).sum((1, 2))[:, None], (o2 * W * ga).sum((1, 2))[:, None],
                              torch.zeros(B, D, dtype=F8)), -1)
            g_x = (o2 * W * h)[..., None] * tk * s
        else:
            phi = nk * x1[:, :, None, :] - nk * x2[:, None, :, :]
            sn = torch.sin(math.pi * phi)
            gg = torch.exp(-2.0 * (tk * sn).square().sum(-1))
            wg = (o2 * W * gg)[..., None]
            g_t = -4.0 * wg * (tk * sn).square() / tk
            g_nu = -2.0 * math.pi * wg * tk ** 2 * phi * torch.sin(2 * math.pi * phi) / nk
            want = torch.cat((g_t.sum((1, 2)), (W * gg).sum((1, 2))[:, None], torch.zeros(B, 1, dtype=F8), g_nu.sum((1, 2))), -1)
            g_x = -2.0 * math.pi * wg * tk ** 2 * nk * torch.sin(2 * math.pi * phi)
    tol = 2e-5 if family == "rq" else 1e-11  # (rq: the three-term series, 5e-5 relative on the near pair's share)
    assert rel(want.numpy(), th.grad.numpy()) < tol
    assert rel(g_x.sum(2).numpy(), x1.grad.numpy()) < 1e-11


def test_attributes_and_the_family_dicts():
    assert list(covariance.PARAM_FAMILIES) == ["rq", "periodic"]
    assert covariance.PARAM_FAMILIES["rq"] is covariance.rq and covariance.PARAM_FAMILIES["periodic"] is covariance.periodic
    assert covariance.rq.native_family == _hip.LO_KERNEL_RQ == 16
    assert covariance.periodic.native_family == _hip.LO_KERNEL_PERIODIC == 17
    assert covariance.rq.native_outputs == covariance.periodic.native_outputs == "param"
    others = set(covariance.FAMILIES) | set(covariance.GRAD_FAMILIES) | set(covariance.TASK_FAMILIES)
    assert not set(covariance.PARAM_FAMILIES) & others
    assert all(f.native_family in (0, 1, 2, 3) for f in covariance.FAMILIES.values())


def test_binding_of_abi_39():
    assert _hip.ABI_VERSION >= 39 and _hip.LO_OP_KERNEL_PARAM_DIAG == 18 and _hip.LO_KERNEL_PARAM_MAX_DIM == 32
    for name, nargs in (("lo_kernel_param_mv_workspace_bytes", 5), ("lo_kernel_param_mv_f32", 16),
                        ("lo_kernel_param_bilinear_workspace_bytes", 5), ("lo_kernel_param_bilinear_f32", 15),
                        ("lo_kernel_param_points_grad_workspace_bytes", 5), ("lo_kernel_param_points_grad_f32", 15)):
        assert name in _hip.EXPORTS and len(_hip._PROTOTYPES[name][1]) == nargs
        stem = name.replace("_param", "")  # (the prototypes of the entry points they are modelled on)
        assert _hip._PROTOTYPES[name] == _hip._PROTOTYPES[stem]
    for name in ("kernel_param_mv", "kernel_param_bilinear", "kernel_param_points_grad", "kernel_param_diag_descriptor",
                 "kernel_param_theta"):
        assert callable(getattr(K, name))
    lib = _hip.load()  # (raises when the library does not export a symbol of the table; the sizers are host code)
    assert lib.lo_abi_version() == _hip.ABI_VERSION
    s = K.OperatorDescriptor(_hip.LO_OP_KERNEL_PARAM_DIAG, 2, 40, R=3, n2=17).c_struct()
    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (18, 0, 17, 3, 40)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lo_amd.h")).read()
    for text in ("#define LO_OP_KERNEL_PARAM_DIAG 18", "#define LO_KERNEL_RQ 16", "#define LO_KERNEL_PERIODIC 17",
                 "#define LO_KERNEL_PARAM_MAX_DIM 32"):
        assert text in header


def test_theta_layout():
    ls, os_ = torch.tensor([[[0.5, 0.25]], [[2.0, 4.0]]]), torch.tensor([2.0, 3.0])
    th = K.kernel_param_theta(ls, os_, (2,), 2, alpha=torch.tensor([1.5, 2.5]))
    assert torch.equal(th, torch.tensor([[2.0, 4.0, 4.0, 1.5, 0.0, 0.0], [0.5, 0.25, 9.0, 2.5, 0.0, 0.0]]))
    th = K.kernel_param_theta(ls[:, :, :1], os_, (2,), 2, period_length=torch.tensor([[[0.5]], [[0.25]]]))
    assert torch.equal(th, torch.tensor([[2.0, 2.0, 4.0, 0.0, 2.0, 2.0], [0.5, 0.5, 9.0, 0.0, 4.0, 4.0]]))


def split_count(B, M, N):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-M // 256), -(-N // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return rb, -(-N // jchunk)


@pytest.mark.parametrize("B,M,N,D,c", [(512, 130, 130, 2, 1), (1, 1, 1, 1, 1), (2, 300, 257, 3, 3), (3, 70, 300, 17, 17),
                                       (1, 16384, 16384, 4, 1), (8, 8192, 8192, 16, 17), (1, 140, 140, 32, 4)])
def test_sizers_are_the_closed_form_of_the_layouts(B, M, N, D, c):
    lib = _hip.load()
    rb, js = split_count(B, M, N)
    assert lib.lo_kernel_param_mv_workspace_bytes(B, M, N, D, c) == 256 + (4 * js * B * M * c if js > 1 else 0)
    assert lib.lo_kernel_param_points_grad_workspace_bytes(B, M, N, D, c) == 256 + (4 * js * B * M * D if js > 1 else 0)
    DP = 4 if D <= 4 else (8 if D <= 8 else (16 if D <= 16 else 32))
    assert lib.lo_kernel_param_bilinear_workspace_bytes(B, M, N, D, c) == 256 + 4 * B * rb * js * (2 * DP + 2)


def test_sizers_return_0_outside_the_limits():
    lib = _hip.load()
    sizers = (lib.lo_kernel_param_mv_workspace_bytes, lib.lo_kernel_param_bilinear_workspace_bytes,
              lib.lo_kernel_param_points_grad_workspace_bytes)
    for args in ((1, 10, 10, 33, 1), (0, 10, 10, 3, 1), (1, 0, 10, 3, 1), (1, 10, 0, 3, 1), (1, 10, 10, 0, 1),
                 (1, 10, 10, 3, 0), (65536, 10, 10, 3, 1), (1, 0x7ffffe01, 10, 3, 1), (1, 10, 0x7ffffe01, 3, 1),
                 (1, 10, 10, 3, 0x80000000)):
        for sizer in sizers:
            assert sizer(*args) == 0, args
    for sizer in sizers:
        assert sizer(1, 10, 10, 32, 1) >= 256 and sizer(65535, 10, 10, 1, 1) >= 256


@pytest.mark.parametrize("fn", [covariance.rq, covariance.periodic], ids=["rq", "periodic"])
def test_every_branch_of_the_gate(fn):
    g = torch.Generator().manual_seed(50)
    x = torch.rand(20, 3, generator=g)
    rq = fn is covariance.rq
    own, other = ("alpha", "period_length") if rq else ("period_length", "alpha")
    ok = param_op(x, fn)
    assert ok._native_param_refusal(check_device=False) is None
    assert "device" in ok._native_param_refusal() and not ok._is_native_param()  # (CPU tensors)
    assert ok._kernel_descriptor() is None
    for D in (1, 32):
        assert param_op(torch.rand(20, D, generator=g), fn)._native_param_refusal(check_device=False) is None
    assert param_op(x, fn, ls=torch.full((1, 1), 0.7))._native_param_refusal(check_device=False) is None  # (shared)
    xb = torch.rand(2, 20, 3, generator=g)
    sh = {"alpha": torch.ones(2)} if rq else {"period_length": torch.ones(2, 1, 1)}
    batched = KernelLinearOperator(xb, xb, fn, num_nonbatch_dimensions=NB, lengthscale=torch.full((2, 1, 3), 0.7),
                                   outputscale=torch.ones(2), **sh)
    assert batched._native_param_refusal(check_device=False) is None
    # the diagonal is outputscale^2 without a call of covar_func

    def never(*a, **k):
        raise AssertionError("covar_func was called")

    never.native_family, never.native_outputs = fn.native_family, "param"
    assert torch.equal(param_op(x, never)._diagonal(), torch.full((20,), 1.1).square())

    def refusal(op):
        return op._native_param_refusal(check_device=False)

    plain = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 3),
                                 outputscale=torch.tensor(1.0))
    assert "native_outputs" in refusal(plain)

    def wrong_family(x1, x2, **params):
        return fn(x1, x2, **params)

    wrong_family.native_outputs, wrong_family.native_family = "param", _hip.LO_KERNEL_RBF
    assert "native_family" in refusal(param_op(x, wrong_family, **{own: torch.tensor(1.0)}))
    assert "one output per input" in refusal(param_op(x, fn, num_outputs_per_input=(2, 2)))
    assert "parameters other than" in refusal(param_op(x, fn, extra=torch.ones(1)))
    assert "parameters other than" in refusal(param_op(x, fn, flag=True))
    assert "parameters other than" in refusal(param_op(x, fn, drop=(own,)))
    swapped = {"alpha": torch.tensor(1.0)} if other == "alpha" else {"period_length": torch.ones(1, 3)}
    assert "parameters other than" in refusal(param_op(x, fn, drop=(own,), **swapped))  # (the other family's parameter)
    assert "D = 33" in refusal(param_op(torch.rand(20, 33, generator=g), fn))
    assert "D = 0" in refusal(param_op(torch.zeros(20, 0), fn))
    assert "D = " in refusal(param_op(x, fn, x2=torch.rand(20, 4, generator=g), ls=torch.ones(1, 1),
                                      **({} if rq else {"period_length": torch.ones(1, 1)})))
    assert "lengthscale" in refusal(param_op(x, fn, ls=torch.ones(1, 2)))
    assert "lengthscale" in refusal(param_op(x, fn, ls=torch.ones(3), nb={**NB, "lengthscale": 1}))
    assert "outputscale" in refusal(param_op(x, fn, nb={"alpha": 0}, outputscale=torch.ones(1, 1)))
    if rq:
        assert "alpha" in refusal(param_op(x, fn, alpha=torch.ones(1, 1), nb={"outputscale": 0}))
    else:
        assert "period_length" in refusal(param_op(x, fn, period_length=torch.ones(1, 2)))
        assert "period_length" in refusal(param_op(x, fn, period_length=torch.ones(3), nb={**NB, "period_length": 1}))
    assert "float32" in refusal(param_op(x.double(), fn, dtype=F8))
    assert "float32" in refusal(param_op(x, fn, **{own: (torch.tensor(1.0, dtype=F8) if rq else torch.ones(1, 3, dtype=F8))}))


@pytest.mark.parametrize("fn", [covariance.rq, covariance.periodic], ids=["rq", "periodic"])
def test_the_other_gates_stay_out(fn):
    """`_native_refusal` (and its float64 twin) keep answering "parameters other than lengthscale and outputscale", so the
    fused kernel sum, the Kronecker multitask kind and the LMC kind never take such an operator; the task and gradient
    gates refuse it; the param gate refuses the plain families."""
    from linear_operator_amd.operators.sum_linear_operator import _kernel_group_pair, _kernel_groups, _lmc_terms

    x = torch.rand(20, 3, generator=torch.Generator().manual_seed(51))
    op = param_op(x, fn)
    why = "parameters other than lengthscale and outputscale"
    assert op._native_refusal(check_device=False) == why and op._native_refusal() == why
    assert param_op(x.double(), fn, dtype=F8)._native_f64_refusal(check_device=False) == why
    assert "native_outputs" in op._native_task_refusal(check_device=False)
    assert "native_outputs" in op._native_grad_refusal(check_device=False)
    assert not (op._is_native() or op._is_native_f64() or op._is_native_grad() or op._is_native_task())
    plain = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 3),
                                 outputscale=torch.tensor(1.0))
    assert _kernel_group_pair([op, op]) is None and _kernel_group_pair([plain, op]) is None
    assert _kernel_groups([plain, op, plain], check_device=False) == [[plain, plain], op]  # (a term of its own)
    kron = KroneckerProductLinearOperator(op, DenseLinearOperator(torch.eye(2)))
    assert kron._kernel_kron_refusal(check_device=False) is not None and kron._kernel_descriptor() is None
    assert _lmc_terms([kron, kron], check_device=False) is None
    assert SumLinearOperator(op, plain)._kernel_descriptor() is None  # (CPU tensors: nothing lowers)


@pytest.mark.parametrize("p", list(CASES))
def test_dense_path_on_the_cpu_reproduces_the_goldens(p):
    """The fixtures' inputs on the CPU (outside the gate's device condition: covar_func is evaluated densely): float32
    against the reference's float32 values within 4 x its own error, float64 against the float64 values."""
    G = np.load(os.path.join(HERE, "golden", f"g47_kernel_param_{p}.npz"))
    B, n, D, seed = CASES[p]
    fn, shape = covariance.PARAM_FAMILIES[p], SHAPE[p]
    assert max(G["gcond"]) <= 750.0

    def build(t):
        return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions=NB, lengthscale=t["lengthscale"],
                                    outputscale=t["outputscale"], **{shape: t[shape]})

    for dtype, tol in ((torch.float32, None), (F8, 1e-10)):
        t = {k: torch.from_numpy(v).to(dtype) for k, v in inputs(p).items()}
        for k in grad_names(p):
            t[k].requires_grad_(True)
        op = build(t)
        assert op.shape == (B, n, n)
        bound = lambda q: tol if tol else 4.0 * max(float(G[q + "_err"]), 1e-7)  # noqa: E731
        assert rel((op @ t["V"]).detach().numpy(), G["mv_64"]) <= bound("mv")
        assert rel((op.mT @ t["V"]).detach().numpy(), G["mv_64"]) <= bound("mv")
        assert rel(op.diagonal().detach().numpy(), G["diag_64"]) <= bound("diag")
        sub = op[..., 3:40, 17:90]
        assert isinstance(sub, KernelLinearOperator) and sub.shape == (B, 37, 73)
        A = AddedDiagLinearOperator(op, DiagLinearOperator(t["noise"]))
        with settings.fast_computations(solves=False, log_prob=False, covar_root_decomposition=False):
            iq = A.inv_quad(t["rhs"])
        iq.sum().backward()
        assert rel(iq.detach().numpy(), G["iq_64"]) <= bound("iq")
        for q, k in (("gl", "lengthscale"), ("go", "outputscale"), ("gs", shape), ("gx", "x")):
            assert rel(t[k].grad.numpy(), G[q + "_64"]) <= bound(q), (q, str(dtype))
