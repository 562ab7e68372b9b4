"""The matrix-free RBF gradient kernel (a GP with derivative observations, D + 1 outputs per input) without a GPU: the
binding of ABI 30 (symbols, constants, the host-side sizers against the closed form of their layouts),
covariance.rbf_grad block by block against float64 autograd of covariance.rbf, the gate `_native_grad_refusal` decided on
CPU tensors through its `check_device=False` form (with `_native_refusal` answering what it always did), the CPU general
path against the reference's goldens (tests/golden/g41_kernel_grad_*.npz), the closed-form diagonal, the transpose and
slicing by whole points."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_grad import CASES, ERR_FLOOR, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import DenseLinearOperator, KernelLinearOperator  # noqa: E402

REF_FACTOR = 4.0
NB = {"outputscale": 0}


def grad_op(x, x2=None, dtype=torch.float32, fn=covariance.rbf_grad, outputs=None, ls=None, **extra):
    D = x.shape[-1]
    ls = torch.linspace(0.5, 0.9, D, dtype=dtype).reshape(1, D) if ls is None else ls
    return KernelLinearOperator(x, x if x2 is None else x2, fn, num_nonbatch_dimensions=NB,
                                num_outputs_per_input=(D + 1, D + 1) if outputs is None else outputs,
                                lengthscale=ls, outputscale=torch.tensor(1.1, dtype=dtype), **extra)


def split_count(B, M, N):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-M // 256), -(-N // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return rb, -(-N // jchunk)


def test_binding_of_abi_30():
    assert _hip.ABI_VERSION >= 30 and _hip.LO_OP_KERNEL_GRAD_DIAG == 14 and _hip.LO_KERNEL_GRAD_MAX_DIM == 16
    for name, nargs in (("lo_kernel_grad_mv_workspace_bytes", 5), ("lo_kernel_grad_mv_f32", 16),
                        ("lo_kernel_grad_bilinear_workspace_bytes", 5), ("lo_kernel_grad_bilinear_f32", 15)):
        assert name in _hip.EXPORTS and len(_hip._PROTOTYPES[name][1]) == nargs
    assert callable(K.kernel_grad_diag_descriptor) and callable(K.kernel_grad_mv) and callable(K.kernel_grad_bilinear)
    lib = _hip.load()  # (raises when the library does not export a symbol of the table; the sizers are host code)
    assert lib.lo_abi_version() >= 30
    # the struct of the kind: no new member, nterms stays 0, the family rides in n2, N = n (D + 1)
    desc = K.OperatorDescriptor(_hip.LO_OP_KERNEL_GRAD_DIAG, 2, 40, R=3, n2=0)
    s = desc.c_struct()
    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (14, 0, 0, 3, 40)
    assert covariance.rbf_grad.native_family == _hip.LO_KERNEL_RBF and covariance.rbf_grad.native_outputs == "grad"
    assert covariance.GRAD_FAMILIES == {"rbf_grad": covariance.rbf_grad} and "rbf_grad" not in covariance.FAMILIES
    assert all(getattr(f, "native_outputs", None) is None for f in covariance.FAMILIES.values())


@pytest.mark.parametrize("B,M,N,D,c", [(512, 40, 40, 2, 2), (1, 1, 1, 1, 1), (1, 257, 257, 3, 17), (3, 130, 70, 16, 1),
                                       (1, 16384, 16384, 3, 1), (8, 1024, 1024, 8, 17)])
def test_sizers_are_the_closed_form_of_the_layouts(B, M, N, D, c):
    """Product: the tail alone without a split, else js copies of y [B, M (D + 1), c].  Bilinear: one partial of DP + 1
    floats per workgroup."""
    lib = _hip.load()
    rb, js = split_count(B, M, N)
    assert lib.lo_kernel_grad_mv_workspace_bytes(B, M, N, D, c) == 256 + (4 * js * B * M * (D + 1) * c if js > 1 else 0)
    DP = 4 if D <= 4 else (8 if D <= 8 else 16)
    assert lib.lo_kernel_grad_bilinear_workspace_bytes(B, M, N, D, c) == 256 + 4 * B * rb * js * (DP + 1)
    assert (js == 1) == (B == 512 or N <= 128)  # (workgroups enough, or one tile: no split)


def test_sizers_refuse_what_the_entry_points_refuse():
    lib = _hip.load()
    for args in ((1, 10, 10, 17, 1), (0, 10, 10, 3, 1), (1, 0, 10, 3, 1), (1, 10, 0, 3, 1), (1, 10, 10, 0, 1),
                 (1, 10, 10, 3, 0), (65536, 10, 10, 3, 1)):
        assert lib.lo_kernel_grad_mv_workspace_bytes(*args) == 0, args
        assert lib.lo_kernel_grad_bilinear_workspace_bytes(*args) == 0, args
    assert lib.lo_kernel_grad_mv_workspace_bytes(1, 10, 10, 16, 1) == 256


def autograd_blocks(x1, x2, ls, os_):
    """The block matrix from float64 autograd of the plain RBF: value, d / dx1, d / dx2, d^2 / dx1 dx2 per pair."""
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    k = covariance.rbf(a, b, ls, os_)
    D, T = x1.shape[-1], x1.shape[-1] + 1
    out = torch.zeros(*k.shape[:-2], k.shape[-2] * T, k.shape[-1] * T, dtype=torch.float64)
    for idx in itertools.product(*[range(s) for s in k.shape]):
        *bi, i, j = idx
        ga, gb = torch.autograd.grad(k[idx], (a, b), create_graph=True)
        out[(*bi, i * T, j * T)] = k[idx]
        for q in range(D):
            out[(*bi, i * T + q + 1, j * T)] = ga[(*bi, i, q)]
            out[(*bi, i * T, j * T + q + 1)] = gb[(*bi, j, q)]
            h, = torch.autograd.grad(ga[(*bi, i, q)], b, retain_graph=True)
            out[(*bi, i * T + q + 1, slice(j * T + 1, (j + 1) * T))] = h[(*bi, j)]
    return out


@pytest.mark.parametrize("batch,M,N,D,shared", [((), 3, 4, 2, False), ((2,), 1, 1, 3, True), ((2, 3), 2, 3, 1, False),
                                                ((2,), 3, 2, 4, True)])
def test_rbf_grad_is_the_block_matrix_of_float64_autograd(batch, M, N, D, shared):
    g = torch.Generator().manual_seed(41)
    f8 = torch.float64
    x1, x2 = torch.randn(*batch, M, D, generator=g, dtype=f8), torch.randn(*batch, N, D, generator=g, dtype=f8)
    ls = torch.rand((*batch, 1, 1 if shared else D), generator=g, dtype=f8) + 0.5
    os_ = torch.rand(batch, generator=g, dtype=f8) + 0.5
    got = covariance.rbf_grad(x1, x2, ls, os_)
    assert got.shape == (*batch, M * (D + 1), N * (D + 1))
    assert (got - autograd_blocks(x1, x2, ls, os_)).abs().max() < 1e-13
    # K(x2, x1) is the transpose, and float32 inputs give a float32 matrix
    assert torch.equal(covariance.rbf_grad(x2, x1, ls, os_), got.mT)
    assert covariance.rbf_grad(x1.float(), x2.float(), ls.float(), os_.float()).dtype == torch.float32


def test_rbf_grad_survives_the_pairs_as_a_batch_dimension():
    """The call pattern of `_diagonal` and `_get_indices`: x as [n, *b, 1, D] with M = N = 1, the parameters with one more
    leading dimension; and the lengthscale's gradient flows (plain differentiable torch)."""
    g = torch.Generator().manual_seed(42)
    x = torch.rand(2, 5, 3, generator=g, dtype=torch.float64)
    ls = (torch.rand(2, 1, 3, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    os_ = torch.rand(2, generator=g, dtype=torch.float64) + 0.5
    a = x.movedim(-2, 0).unsqueeze(-2)
    blocks = covariance.rbf_grad(a, a, ls.unsqueeze(0), os_.unsqueeze(0))
    assert blocks.shape == (5, 2, 4, 4)
    full = covariance.rbf_grad(x, x, ls, os_)
    for i in range(5):
        assert torch.allclose(blocks[i], full[:, 4 * i: 4 * i + 4, 4 * i: 4 * i + 4], atol=1e-15)
    full.sum().backward()
    assert ls.grad is not None and bool(ls.grad.abs().sum() > 0)


def test_gate_on_cpu_tensors():
    more = "more than one output per input"
    for D in (1, 16):
        ok = grad_op(torch.rand(20, D))
        assert ok._native_grad_refusal(check_device=False) is None
        assert "device" in ok._native_grad_refusal()  # (CPU tensors: the full gate refuses, nothing lowers)
        assert ok._kernel_descriptor() is None and not ok._is_native_grad()
        assert ok._native_refusal(check_device=False) == more
    shared = grad_op(torch.rand(20, 3), ls=torch.full((1, 1), 0.7))
    assert shared._native_grad_refusal(check_device=False) is None
    x = torch.rand(20, 3)
    wide = grad_op(torch.rand(20, 17))
    assert "LO_KERNEL_GRAD_MAX_DIM" in wide._native_grad_refusal(check_device=False)
    assert wide._native_refusal(check_device=False) == more
    one = grad_op(x, outputs=(1, 1))  # (D + 1 outputs declared as one: not this gate's operator)
    assert "num_outputs_per_input" in one._native_grad_refusal(check_device=False)
    plain = grad_op(x, fn=covariance.rbf)  # (D + 1, D + 1) with the one-output family
    assert "native_outputs" in plain._native_grad_refusal(check_device=False)
    assert plain._native_refusal(check_device=False) == more
    plain11 = grad_op(x, fn=covariance.rbf, outputs=(1, 1))  # the plain operator: its own gate, not this one
    assert plain11._native_refusal(check_device=False) is None
    assert "native_outputs" in plain11._native_grad_refusal(check_device=False)
    extra = grad_op(x, fn=lambda a, b, lengthscale, outputscale, period: covariance.rbf_grad(a, b, lengthscale, outputscale),
                    period=torch.tensor(1.0))
    assert "native_outputs" in extra._native_grad_refusal(check_device=False)  # (a wrapper carries no attributes)

    def with_period(a, b, lengthscale, outputscale, period):
        return covariance.rbf_grad(a, b, lengthscale, outputscale)

    with_period.native_family, with_period.native_outputs = _hip.LO_KERNEL_RBF, "grad"
    extra = grad_op(x, fn=with_period, period=torch.ones(1, 1))
    assert "parameters other than" in extra._native_grad_refusal(check_device=False)
    assert extra._native_refusal(check_device=False) == more

    def matern_grad(a, b, lengthscale, outputscale):
        return covariance.rbf_grad(a, b, lengthscale, outputscale)

    matern_grad.native_family, matern_grad.native_outputs = _hip.LO_KERNEL_MATERN52, "grad"
    assert "other than RBF" in grad_op(x, fn=matern_grad)._native_grad_refusal(check_device=False)
    dbl = grad_op(x.double(), dtype=torch.float64)
    assert dbl._native_grad_refusal(check_device=False) == "not float32"
    assert dbl._native_refusal(check_device=False) == more
    two = grad_op(x, ls=torch.full((1, 2), 0.7))  # neither ARD over the 3 dimensions nor shared
    assert "lengthscale of shape" in two._native_grad_refusal(check_device=False)


def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g41_kernel_grad_{p}.npz"))


def tensors(p, grad=False):
    t = {k: torch.from_numpy(v) for k, v in inputs(p).items()}
    if grad:
        for k in ("lengthscale", "outputscale"):
            t[k].requires_grad_(True)
    return t


def case_op(p, t):
    D = CASES[p][2]
    return KernelLinearOperator(t["x"], t["x"], covariance.rbf_grad, num_outputs_per_input=(D + 1, D + 1),
                                num_nonbatch_dimensions=NB, lengthscale=t["lengthscale"], outputscale=t["outputscale"])


def check(G, p, q, value):
    err, ref_err = rel(value.detach().double().numpy(), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_grad cpu {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


@pytest.mark.parametrize("p", list(CASES))
def test_general_path_against_the_goldens(p):
    """mv, diag and the gradients of a bilinear form on the CPU (the general path: covar_func evaluated densely).  gl / go
    of the fixture are gradients of inv_quad(rhs) = -(solve^T dK solve): the bilinear derivative at the float64 solve."""
    G = golden(p)
    B, n, D, seed = CASES[p]
    t = tensors(p)
    S = case_op(p, t)
    assert S.shape == (B, n * (D + 1), n * (D + 1))
    check(G, p, "mv", S @ t["V"])
    check(G, p, "diag", S.diagonal())
    tg = tensors(p, grad=True)
    sol = torch.from_numpy(G["solve_64"]).float()
    grads = case_op(p, tg)._bilinear_derivative(sol, -sol)
    assert grads[0] is None and grads[1] is None  # (the points ask for no gradient)
    names = list(case_op(p, tg)._differentiable_kwargs)
    by_name = dict(zip(names, grads[2:]))
    check(G, p, "gl", by_name["lengthscale"])
    check(G, p, "go", by_name["outputscale"])


@pytest.mark.parametrize("p", list(CASES))
def test_closed_form_diagonal_equals_the_covar_func_one(p):
    t = tensors(p, grad=True)
    S = case_op(p, t)
    assert S._native_grad_refusal(check_device=False) is None

    def guarded(*a, **k):
        raise AssertionError("covar_func was called")

    guarded.native_family, guarded.native_outputs = _hip.LO_KERNEL_RBF, "grad"
    D = CASES[p][2]
    closed = KernelLinearOperator(t["x"], t["x"], guarded, num_outputs_per_input=(D + 1, D + 1), num_nonbatch_dimensions=NB,
                                  lengthscale=t["lengthscale"], outputscale=t["outputscale"])._diagonal()
    dense = covariance.rbf_grad(t["x"], t["x"], t["lengthscale"], t["outputscale"]).diagonal(dim1=-2, dim2=-1)
    assert closed.shape == dense.shape and torch.allclose(closed, dense, rtol=1e-6, atol=0)
    # outside the gate (float64) the pairs go through covar_func, with the same result
    t64 = {k: v.detach().double() for k, v in t.items()}
    general = case_op(p, t64)
    assert general._native_grad_refusal(check_device=False) == "not float32"
    assert torch.allclose(general._diagonal(), dense.double(), rtol=1e-6, atol=0)
    # and the closed form is differentiable in the hyperparameters
    closed.sum().backward()
    assert t["lengthscale"].grad is not None and t["outputscale"].grad is not None


def test_transpose_and_rectangular_operator():
    g = torch.Generator().manual_seed(43)
    x1, x2 = torch.rand(7, 3, generator=g), torch.rand(5, 3, generator=g)
    S = grad_op(x1, x2)
    assert S.shape == (28, 20) and S.mT.shape == (20, 28)
    assert S._native_grad_refusal(check_device=False) is None and S.mT._native_grad_refusal(check_device=False) is None
    dense = S.to_dense()
    assert torch.equal(S.mT.to_dense(), dense.mT)
    v = torch.randn(28, 2, generator=g)
    assert torch.allclose(S._t_matmul(v), dense.mT @ v, atol=1e-5)
    assert torch.allclose(S[3:6, 2:9].to_dense(), dense[3:6, 2:9])


def test_slices_of_whole_points_stay_inside_the_gate():
    g = torch.Generator().manual_seed(44)
    x = torch.rand(2, 9, 3, generator=g)
    t = dict(lengthscale=torch.rand(2, 1, 3, generator=g) + 0.5, outputscale=torch.rand(2, generator=g) + 0.5)
    S = KernelLinearOperator(x, x, covariance.rbf_grad, num_outputs_per_input=(4, 4), num_nonbatch_dimensions=NB, **t)
    dense = S.to_dense()
    whole = S[:, 8:24, 8:24]  # points 2 .. 5 on both sides
    assert isinstance(whole, KernelLinearOperator) and whole.shape == (2, 16, 16)
    assert whole._native_grad_refusal(check_device=False) is None and whole._same_points()
    assert whole.x1.shape == (2, 4, 3) and torch.equal(whole.to_dense(), dense[:, 8:24, 8:24])
    rect = S[:, 4:12, :]  # whole points, two different ranges: still the operator, no longer one points tensor
    assert isinstance(rect, KernelLinearOperator) and rect.shape == (2, 8, 36) and not rect._same_points()
    assert torch.equal(rect.to_dense(), dense[:, 4:12, :])
    member = S[1, 4:12, 4:12]
    assert isinstance(member, KernelLinearOperator) and member.shape == (8, 8)
    assert member._native_grad_refusal(check_device=False) is None
    assert torch.equal(member.to_dense(), dense[1, 4:12, 4:12])
    for rows, cols in ((slice(1, 9), slice(0, 8)), (slice(0, 8), slice(0, 6)), (slice(0, 16, 2), slice(0, 8)),
                       (slice(0, 8), torch.tensor([0, 1, 2, 3]))):
        part = S[(slice(None), rows, cols)]  # not whole points (or stepped, or a tensor index): indexed densely, as before
        assert isinstance(part, DenseLinearOperator)
        assert torch.equal(part.to_dense(), dense[(slice(None), rows, cols)])
    # outside the gate nothing changes: any other several-output operator is indexed densely even by whole points
    other = KernelLinearOperator(x, x, lambda a, b, **kw: covariance.rbf_grad(a, b, **kw), num_outputs_per_input=(4, 4),
                                 num_nonbatch_dimensions=NB, **t)
    assert isinstance(other[:, 8:24, 8:24], DenseLinearOperator)
