"""The spectral mixture kernel without a GPU: covariance.spectral_mixture against an independent float64 double loop, its
Q = 1, mu = 0 identity with covariance.rbf, the derivative formulas of csrc/lo_kernel_sm.hip against
float64 autograd (a pair with mu tau = 1/4 included: the no-division rule), the binding of ABI 40 (symbols, constants, the
host-side sizers), every branch of the gate `_native_sm_refusal` decided on CPU tensors through its `check_device=False`
form (with the other five gates answering what they always did), and the dense path on the CPU against the goldens."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_sm import CASES, GRADS, NB, PARAMS, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, SumLinearOperator)
from linear_operator_amd.operators import kernel_linear_operator as klo  # noqa: E402

F8 = torch.float64
FN = covariance.spectral_mixture


def rand(g, *shape, lo=0.5, hi=1.5, dtype=F8):
    return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=dtype)


def sm_op(x, fn=FN, x2=None, dtype=torch.float32, Q=3, nb=NB, drop=(), num_outputs_per_input=(1, 1), **extra):
    D = x.shape[-1]
    batch = x.shape[:-2]
    params = {"mixture_weights": torch.linspace(0.4, 0.9, Q, dtype=dtype).expand(*batch, Q),
              "mixture_means": torch.full((*batch, Q, D), 0.7, dtype=dtype),
              "mixture_scales": torch.full((*batch, Q, D), 0.3, dtype=dtype)}
    params.update(extra)
    for k in drop:
        del params[k]
    return KernelLinearOperator(x, x if x2 is None else x2, fn, num_outputs_per_input=num_outputs_per_input,
                                num_nonbatch_dimensions=nb, **params)


def plain_op(x, fn=covariance.rbf, **extra):
    return KernelLinearOperator(x, x, fn, num_nonbatch_dimensions={"outputscale": 0, "alpha": 0},
                                lengthscale=torch.ones(1, x.shape[-1]), outputscale=torch.tensor(1.0), **extra)


def test_spectral_mixture_is_the_double_loop():
    """Entry by entry in float64 (math.*, not torch), rectangular and batched, and the leading-batch call pattern."""
    g = torch.Generator().manual_seed(48)
    n, m, D, Q = 5, 4, 3, 2
    x1, x2 = 3.0 * torch.rand(2, n, D, generator=g, dtype=F8), 3.0 * torch.rand(2, m, D, generator=g, dtype=F8)
    w, mu, sg = rand(g, 2, Q), rand(g, 2, Q, D, lo=0.2, hi=1.2), rand(g, 2, Q, D, lo=0.1, hi=0.4)
    got = FN(x1, x2, w, mu, sg)
    assert got.shape == (2, n, m) and got.dtype == F8
    for b in range(2):
        for i in range(n):
            for j in range(m):
                want = 0.0
                for q in range(Q):
                    tau = [float(x1[b, i, k]) - float(x2[b, j, k]) for k in range(D)]
                    env = math.exp(-2.0 * math.pi ** 2 * sum((float(sg[b, q, k]) * tau[k]) ** 2 for k in range(D)))
                    osc = math.prod(math.cos(2.0 * math.pi * float(mu[b, q, k]) * tau[k]) for k in range(D))
                    want += float(w[b, q]) * env * osc
                assert abs(float(got[b, i, j]) - want) <= 1e-13 * max(1.0, abs(want)), (b, i, j)
    assert FN(x1.float(), x2.float(), w.float(), mu.float(), sg.float()).dtype == torch.float32
    assert torch.allclose(FN(x1[0], x2[0], w[0], mu[0], sg[0]), got[0], rtol=1e-14)  # (no batch at all)
    # the call pattern of `_diagonal` / `_get_indices`: the pairs as a leading batch dimension; the diagonal is sum_q w_q
    a = x1.movedim(-2, 0).unsqueeze(-2)
    blocks = FN(a, a, w.unsqueeze(0), mu.unsqueeze(0), sg.unsqueeze(0))
    assert blocks.shape == (n, 2, 1, 1)
    assert torch.allclose(blocks[..., 0, 0].movedim(0, -1), w.sum(-1)[:, None].expand(2, n), rtol=1e-14)
    b2 = x2.movedim(-2, 0).unsqueeze(-2)[:n - 1]
    pairs = FN(a[:n - 1], b2, w.unsqueeze(0), mu.unsqueeze(0), sg.unsqueeze(0))[..., 0, 0].movedim(0, -1)
    assert torch.allclose(pairs, got[:, :n - 1, :n - 1].diagonal(dim1=-2, dim2=-1), rtol=1e-13)


def test_one_mixture_with_zero_means_is_rbf():
    """Q = 1, mu = 0: w exp(-2 pi^2 sum (sigma tau)^2) = os^2 exp(-r^2 / 2) with l = 1 / (2 pi sigma), os = sqrt(w)."""
    g = torch.Generator().manual_seed(49)
    x, x2 = torch.rand(2, 9, 3, generator=g, dtype=F8), torch.rand(2, 7, 3, generator=g, dtype=F8)
    w, sg = rand(g, 2, 1), rand(g, 2, 1, 3, lo=0.1, hi=0.6)
    got = FN(x, x2, w, torch.zeros(2, 1, 3, dtype=F8), sg)
    want = covariance.rbf(x, x2, 1.0 / (2.0 * math.pi * sg), w[:, 0].sqrt())
    assert rel(got.numpy(), want.numpy()) < 1e-14


def test_derivative_formulas_against_fp64_autograd():
    """The per-pair formulas the kernels accumulate, summed with random weights W in float64, against autograd
    of the dense function.  One pair has mu tau = 1/4 exactly in every coordinate of mixture 0: its cosines are 0 (to
    rounding), the case the prefix / suffix products exist for -- a form that divides prod c by c_k fails there."""
    g = torch.Generator().manual_seed(50)
    B, M, N, D, Q = 2, 7, 6, 3, 2
    x1 = 4.0 * torch.rand(B, M, D, generator=g, dtype=F8)
    x2 = 4.0 * torch.rand(B, N, D, generator=g, dtype=F8)
    w, mu, sg = rand(g, B, Q), rand(g, B, Q, D, lo=0.2, hi=1.2), rand(g, B, Q, D, lo=0.05, hi=0.2)
    mu[:, 0, :] = 0.5
    x1[:, 0, :] = 1.25
    x2[:, 1, :] = 1.75
    assert bool((mu[:, 0, :] * (x2[:, 1, :] - x1[:, 0, :]) == 0.25).all())
    for t in (x1, w, mu, sg):
        t.requires_grad_(True)
    W = torch.randn(B, M, N, generator=g, dtype=F8)
    (W * FN(x1, x2, w, mu, sg)).sum().backward()
    with torch.no_grad():
        tau = (x1[:, :, None, :] - x2[:, None, :, :])[:, None]                      # [B, 1, M, N, D]
        at = tau.abs()
        muk, sgk = mu[:, :, None, None, :].abs(), sg[:, :, None, None, :]           # [B, Q, 1, 1, D]
        E = torch.exp(-2.0 * math.pi ** 2 * (sgk * at).square().sum(-1))            # [B, Q, M, N]
        c, s = torch.cos(2.0 * math.pi * muk * at), torch.sin(2.0 * math.pi * muk * at)
        assert float(c[:, 0, 0, 1].abs().max()) < 1e-15  # (the pair with mu tau = 1/4)
        pre = torch.cumprod(torch.cat((torch.ones_like(c[..., :1]), c[..., :-1]), -1), -1)
        suf = torch.flip(torch.cumprod(torch.cat((torch.ones_like(c[..., :1]), torch.flip(c, (-1,))[..., :-1]), -1), -1), (-1,))
        ex, pr = pre * suf, c.prod(-1)                                              # prod_{l != k} c_l, prod c
        WE = W[:, None] * E
        g_w = (WE * pr).sum((-2, -1))
        wq = w[:, :, None, None, None]
        g_sg = (-4.0 * math.pi ** 2) * sg * (wq * (WE * pr)[..., None] * at.square()).sum((2, 3))
        g_mu = (-2.0 * math.pi) * torch.sign(mu) * (wq * WE[..., None] * at * s * ex).sum((2, 3))
        g_x = (torch.sign(tau) * wq * WE[..., None] * ((-4.0 * math.pi ** 2) * sgk.square() * at * pr[..., None]
                                                       - 2.0 * math.pi * muk * s * ex)).sum((1, 3))
    assert rel(g_w.numpy(), w.grad.numpy()) < 1e-12
    assert rel(g_sg.numpy(), sg.grad.numpy()) < 1e-12
    assert rel(g_mu.numpy(), mu.grad.numpy()) < 1e-12
    assert rel(g_x.numpy(), x1.grad.numpy()) < 1e-12
    # the pair's own share of d / d mu is not lost: -2 pi tau s w E prod_{l != k} c_l with every c_l = 0 is 0 for D > 1, and
    # the one-coordinate case keeps -2 pi tau w E exactly where the divided form gives 0 / 0
    x1d, x2d = torch.tensor([[1.25]], dtype=F8), torch.tensor([[1.75]], dtype=F8)
    m1 = torch.tensor([[0.5]], dtype=F8, requires_grad=True)
    FN(x1d, x2d, torch.ones(1, dtype=F8), m1, torch.full((1, 1), 0.1, dtype=F8)).sum().backward()
    want = -2.0 * math.pi * 0.5 * math.exp(-2.0 * math.pi ** 2 * (0.1 * 0.5) ** 2)
    assert abs(float(m1.grad) - want) < 1e-14 and abs(want) > 1.0


def test_attributes_and_the_family_dicts():
    assert list(covariance.MIXTURE_FAMILIES) == ["spectral_mixture"] and covariance.MIXTURE_FAMILIES["spectral_mixture"] is FN
    assert FN.native_outputs == "sm" and not hasattr(FN, "native_family")
    assert "spectral_mixture" in covariance.__all__ and "MIXTURE_FAMILIES" in covariance.__all__
    assert "[Q, 1, D]" in covariance.__doc__
    others = (set(covariance.FAMILIES) | set(covariance.GRAD_FAMILIES) | set(covariance.TASK_FAMILIES)
              | set(covariance.PARAM_FAMILIES))
    assert not set(covariance.MIXTURE_FAMILIES) & others


def test_binding_of_abi_40():
    assert _hip.ABI_VERSION >= 40 and _hip.LO_OP_KERNEL_SM_DIAG == 19
    assert _hip.LO_KERNEL_SM_MAX_DIM == 16 and _hip.LO_KERNEL_SM_MAX_MIX == 16
    for name, nargs in (("lo_kernel_sm_mv_workspace_bytes", 6), ("lo_kernel_sm_mv_f32", 16),
                        ("lo_kernel_sm_bilinear_workspace_bytes", 6), ("lo_kernel_sm_bilinear_f32", 15),
                        ("lo_kernel_sm_points_grad_workspace_bytes", 6), ("lo_kernel_sm_points_grad_f32", 15)):
        assert name in _hip.EXPORTS and len(_hip._PROTOTYPES[name][1]) == nargs
        if name.endswith("_f32"):  # (Q stands where `family` stands in the entry points they are modelled on)
            assert _hip._PROTOTYPES[name] == _hip._PROTOTYPES[name.replace("_sm", "_param")]
    for name in ("kernel_sm_mv", "kernel_sm_bilinear", "kernel_sm_points_grad", "kernel_sm_diag_descriptor", "kernel_sm_theta"):
        assert callable(getattr(K, name))
    lib = _hip.load()  # (raises when the library does not export a symbol of the table; the sizers are host code)
    assert lib.lo_abi_version() == _hip.ABI_VERSION
    s = K.OperatorDescriptor(_hip.LO_OP_KERNEL_SM_DIAG, 2, 40, R=3, n2=4).c_struct()
    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (19, 0, 4, 3, 40)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lo_amd.h")).read()
    for text in ("#define LO_OP_KERNEL_SM_DIAG 19", "#define LO_KERNEL_SM_MAX_DIM 16", "#define LO_KERNEL_SM_MAX_MIX 16",
                 "ABI version (40;", "size_t lo_kernel_sm_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, "
                 "int64_t Q, int64_t c);", "theta [B, Q, 2 D + 1]"):
        assert text in header


def test_theta_layout():
    w = torch.tensor([[2.0, 3.0]])
    mu, sg = torch.tensor([[[0.5, -0.25], [4.0, 8.0]]]), torch.tensor([[[0.1, 0.2], [0.3, 0.4]]])
    th = K.kernel_sm_theta(w, mu, sg, (1,), 2)
    assert torch.equal(th, torch.tensor([[[2.0, 0.5, -0.25, 0.1, 0.2], [3.0, 4.0, 8.0, 0.3, 0.4]]]))
    th = K.kernel_sm_theta(w[0], mu[0], sg[0], (3,), 2)  # (parameters without a batch, broadcast to the batch)
    assert th.shape == (3, 2, 5) and torch.equal(th[2], th[0]) and th.is_contiguous()


def split_count(B, M, N):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-M // 256), -(-N // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return rb, -(-N // jchunk)


@pytest.mark.parametrize("B,M,N,D,Q,c", [(512, 130, 130, 2, 1, 1), (1, 1, 1, 1, 1, 1), (2, 300, 257, 3, 2, 3),
                                         (3, 70, 300, 16, 16, 17), (1, 16384, 16384, 1, 4, 1), (8, 8192, 8192, 4, 4, 17),
                                         (1, 140, 140, 5, 3, 4)])
def test_sizers_are_the_closed_form_of_the_layouts(B, M, N, D, Q, c):
    lib = _hip.load()
    rb, js = split_count(B, M, N)
    assert lib.lo_kernel_sm_mv_workspace_bytes(B, M, N, D, Q, c) == 256 + (4 * js * B * M * c if js > 1 else 0)
    assert lib.lo_kernel_sm_points_grad_workspace_bytes(B, M, N, D, Q, c) == 256 + (4 * js * B * M * D if js > 1 else 0)
    DP = 4 if D <= 4 else (8 if D <= 8 else 16)
    assert lib.lo_kernel_sm_bilinear_workspace_bytes(B, M, N, D, Q, c) == 256 + 4 * B * Q * rb * js * (2 * DP + 1)


def test_sizers_return_0_outside_the_limits():
    lib = _hip.load()
    sizers = (lib.lo_kernel_sm_mv_workspace_bytes, lib.lo_kernel_sm_bilinear_workspace_bytes,
              lib.lo_kernel_sm_points_grad_workspace_bytes)
    for args in ((1, 10, 10, 17, 2, 1), (1, 10, 10, 3, 17, 1), (1, 10, 10, 3, 0, 1), (0, 10, 10, 3, 2, 1), (1, 0, 10, 3, 2, 1),
                 (1, 10, 0, 3, 2, 1), (1, 10, 10, 0, 2, 1), (1, 10, 10, 3, 2, 0), (65536, 10, 10, 3, 2, 1),
                 (1, 0x7ffffe01, 10, 3, 2, 1), (1, 10, 0x7ffffe01, 3, 2, 1), (1, 10, 10, 3, 2, 0x80000000)):
        for sizer in sizers:
            assert sizer(*args) == 0, args
    for sizer in sizers:
        assert sizer(1, 10, 10, 16, 16, 1) >= 256 and sizer(65535, 10, 10, 1, 1, 1) >= 256


def test_every_branch_of_the_gate():
    g = torch.Generator().manual_seed(51)
    x = torch.rand(20, 3, generator=g)
    ok = sm_op(x)
    assert ok._native_sm_refusal(check_device=False) is None
    assert "device" in ok._native_sm_refusal() and not ok._is_native_sm()  # (CPU tensors)
    assert ok._kernel_descriptor() is None
    for D, Q in ((1, 1), (16, 16), (1, 16), (16, 1)):
        assert sm_op(torch.rand(20, D, generator=g), Q=Q)._native_sm_refusal(check_device=False) is None
    assert sm_op(torch.rand(2, 20, 3, generator=g))._native_sm_refusal(check_device=False) is None  # (batched)
    # parameters without the batch of the points are expanded by the constructor
    xb = torch.rand(2, 20, 3, generator=g)
    shared = KernelLinearOperator(xb, xb, FN, num_nonbatch_dimensions=NB, mixture_weights=torch.ones(4),
                                  mixture_means=torch.ones(4, 3), mixture_scales=torch.ones(2, 4, 3))
    assert shared._native_sm_refusal(check_device=False) is None

    def refusal(op):
        return op._native_sm_refusal(check_device=False)

    assert refusal(plain_op(x)) == "covar_func has no native_outputs == 'sm'"
    assert "native_outputs" in refusal(plain_op(x, covariance.rq, alpha=torch.tensor(1.0)))
    assert "one output per input" in refusal(sm_op(x, num_outputs_per_input=(2, 2)))
    assert "parameters other than mixture_weights, mixture_means and mixture_scales" == refusal(sm_op(x, extra=torch.ones(1)))
    assert "parameters other than" in refusal(sm_op(x, flag=True))
    assert "parameters other than" in refusal(sm_op(x, drop=("mixture_scales",)))
    assert "parameters other than" in refusal(sm_op(x, drop=("mixture_means",), lengthscale=torch.ones(1, 3)))
    assert "D = 17 beyond LO_KERNEL_SM_MAX_DIM" == refusal(sm_op(torch.rand(20, 17, generator=g)))
    assert "D = 0" in refusal(sm_op(torch.zeros(20, 0)))
    assert "D = 3" in refusal(sm_op(x, x2=torch.rand(20, 4, generator=g), mixture_means=torch.ones(3, 1),
                                    mixture_scales=torch.ones(3, 1)))
    assert "Q = 17 beyond LO_KERNEL_SM_MAX_MIX" == refusal(sm_op(x, Q=17))
    assert "mixture_weights" in refusal(sm_op(x, nb={}, mixture_weights=torch.ones(1, 3)))  # (2 non-batch dimensions)
    assert "mixture_means" in refusal(sm_op(x, mixture_means=torch.ones(3, 1)))  # (GPyTorch's [Q, 1, D] squeezed wrongly)
    assert "mixture_means" in refusal(sm_op(x, mixture_means=torch.ones(2, 3)))  # (another Q)
    assert "mixture_scales" in refusal(sm_op(x, mixture_scales=torch.ones(3, 1)))
    assert "mixture_scales" in refusal(sm_op(x, mixture_scales=torch.ones(3), nb={**NB, "mixture_scales": 1}))
    assert "float32" in refusal(sm_op(x.double(), dtype=F8))
    assert "float32" in refusal(sm_op(x, mixture_weights=torch.ones(3, dtype=F8)))
    assert "float32" in refusal(sm_op(x, x2=x.double()))


def test_the_other_gates_refuse_with_their_existing_strings():
    """The five gates of the family-coded rows answer an SM operator as they answer any covar_func without a family or with
    another tag, so the fused kernel sum, the Kronecker multitask kind and the LMC kind never take one."""
    from linear_operator_amd.operators.sum_linear_operator import _kernel_group_pair, _kernel_groups, _lmc_terms

    x = torch.rand(20, 3, generator=torch.Generator().manual_seed(52))
    op = sm_op(x)
    for check_device in (False, True):
        assert op._native_refusal(check_device) == "covar_func has no native_family"
        assert op._native_grad_refusal(check_device) == "covar_func has no native_outputs == 'grad'"
        assert op._native_task_refusal(check_device) == "covar_func has no native_outputs == 'task'"
        assert op._native_param_refusal(check_device) == "covar_func has no native_outputs == 'param'"
    assert sm_op(x.double(), dtype=F8)._native_f64_refusal(check_device=False) == "covar_func has no native_family"
    assert not (op._is_native() or op._is_native_f64() or op._is_native_grad() or op._is_native_task()
                or op._is_native_param())
    plain = plain_op(x)
    assert _kernel_group_pair([op, op]) is None and _kernel_group_pair([plain, op]) is None
    assert _kernel_groups([plain, op, plain], check_device=False) == [[plain, plain], op]  # (a term of its own)
    kron = KroneckerProductLinearOperator(op, DenseLinearOperator(torch.eye(2)))
    assert kron._kernel_kron_refusal(check_device=False) is not None and kron._kernel_descriptor() is None
    assert _lmc_terms([kron, kron], check_device=False) is None
    assert SumLinearOperator(op, plain)._kernel_descriptor() is None  # (CPU tensors: nothing lowers)


def test_the_resolver_and_the_tables():
    x = torch.rand(20, 3, generator=torch.Generator().manual_seed(53))
    op = sm_op(x)
    row = op._native_variant(check_device=False)
    assert row is klo.MIXTURE_VARIANTS[0] and row.tag == "sm" and row.gate == "_native_sm_refusal"
    assert op._native_variant() is None  # (on the host the device condition refuses)
    assert len(klo.MIXTURE_VARIANTS) == 1 and row not in klo.VARIANTS
    assert [v.gate for v in klo.VARIANTS] == ["_native_refusal", "_native_f64_refusal", "_native_grad_refusal",
                                              "_native_task_refusal", "_native_param_refusal"]
    assert all(v.params is None and v.max_mix is None for v in klo.VARIANTS)  # (the five rows keep their defaults)
    xt = torch.cat((x, torch.zeros(20, 1)), -1)
    others = [plain_op(x), plain_op(x, covariance.rq, alpha=torch.tensor(1.0)),
              plain_op(x, covariance.periodic, period_length=torch.ones(1, 3)),
              KernelLinearOperator(xt, xt, covariance.rbf_task, num_nonbatch_dimensions={"outputscale": 0},
                                   lengthscale=torch.ones(1, 3), outputscale=torch.tensor(1.0), task_covar=torch.eye(2)),
              KernelLinearOperator(x, x, covariance.rbf_grad, num_outputs_per_input=(4, 4),
                                   num_nonbatch_dimensions={"outputscale": 0}, lengthscale=torch.ones(1, 3),
                                   outputscale=torch.tensor(1.0))]
    for other in others:
        got = other._native_variant(check_device=False)
        assert got is not None and got is not row and got in klo.VARIANTS
        assert other._native_sm_refusal(check_device=False) == "covar_func has no native_outputs == 'sm'"


def test_the_diagonal_never_calls_covar_func():
    def never(*a, **k):
        raise AssertionError("covar_func was called")

    never.native_outputs = "sm"
    x = torch.rand(2, 20, 3, generator=torch.Generator().manual_seed(54))
    op = sm_op(x, never, Q=4)
    assert torch.equal(op._diagonal(), op.tensor_params["mixture_weights"].sum(-1, keepdim=True).expand(2, 20))
    assert op.diagonal().shape == (2, 20)


@pytest.mark.parametrize("p", list(CASES))
def test_dense_path_on_the_cpu_reproduces_the_goldens(p):
    """The fixtures' inputs on the CPU (outside the gate's device condition: covar_func is evaluated densely): float32
    against the reference's float32 values within 4 x its own error, float64 against the float64 values."""
    G = np.load(os.path.join(HERE, "golden", f"g48_kernel_sm_{p}.npz"))
    B, n, D, Q, seed = CASES[p]
    assert max(G["gcond"]) <= 750.0

    def build(t):
        return KernelLinearOperator(t["x"], t["x"], FN, num_nonbatch_dimensions=NB, **{k: t[k] for k in PARAMS})

    for dtype, tol in ((torch.float32, None), (F8, 1e-10)):
        t = {k: torch.from_numpy(v).to(dtype) for k, v in inputs(p).items()}
        for k in GRADS.values():
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
        for q, k in GRADS.items():
            assert rel(t[k].grad.numpy(), G[q + "_64"]) <= bound(q), (q, str(dtype))
