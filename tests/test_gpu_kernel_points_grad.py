"""The points' gradient of KernelLinearOperator on the MI355X: lo_kernel_points_grad_f32 (k_kernel_pgrad,
csrc/lo_kernel_op.hip) directly, behind _bilinear_derivative and through the public API, against float64 autograd of the
covariance functions with x1 and x2 as separate leaves.

Bound (the convention of test_gpu_kernel_op.py): rel(got, want) <= REF_FACTOR * max(err32, ERR_FLOOR), err32 the error of
float32 torch autograd of the same function on the same inputs, measured here.  Every test prints the ratio it measured
(DESIGN.md section 6l holds the table)."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_op import ERR_FLOOR, rel, solver_settings  # noqa: E402
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
FAMILY_NAMES = ["rbf", "matern12", "matern32", "matern52"]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(DEV).to(dtype).contiguous()  # (a numpy scalar stays 0-dimensional)


def host(t):
    return t.detach().double().cpu().numpy()


def make_points(seed, B, M, N, D, ard, kind="plain", same=None):
    """The inputs of test_gpu_kernel_op.make_points; `same`: x2 is x1 (default: whenever M == N)."""
    g = rng(seed)
    same = M == N if same is None else same
    x1 = g.random((B, M, D)).astype(np.float32)
    x2 = x1 if same else g.random((B, N, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with r = 0 off the diagonal
        x1 = x1.copy()
        x1[:, 1::2] = x1[:, : x1[:, 1::2].shape[1] * 2: 2]
        x2 = x1 if same else x2
    if kind == "far":  # separations of tens of lengthscales: exp underflows to 0
        x1 = (x1 * 4000.0).astype(np.float32)
        x2 = x1 if same else (x2 * 4000.0).astype(np.float32)
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    return x1, x2, ls, os_


def never_called(fn):
    """A covar_func of the same native family that must not be evaluated."""
    def covar(*args, **kwargs):
        raise AssertionError("covar_func was called")

    covar.native_family = fn.native_family
    return covar


def no_dense():
    return mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation"))


def autograd_points(fn, x1, x2, ls, os_, U, V, dtype):
    """d / d x1 and d / d x2 of sum_s u_s^T K v_s by torch autograd in `dtype`, x1 and x2 separate leaves."""
    a, b = dev(x1, dtype).requires_grad_(True), dev(x2, dtype).requires_grad_(True)
    (dev(U, dtype) * (fn(a, b, dev(ls, dtype), dev(os_, dtype)) @ dev(V, dtype))).sum().backward()
    return host(a.grad), host(b.grad)


def within_bound(label, got, want, ref32):
    err, ref_err = rel(host(got), want), max(rel(ref32, want), ERR_FLOOR)
    print(f"kernel_points_grad {label}: err {err:.3e} torch fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert torch.isfinite(got).all(), label
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def native_both_sides(fn, tx1, tx2, ls, os_, tU, tV):
    theta = K.kernel_theta(dev(ls), dev(os_), (ls.shape[0],), tx1.shape[-1])
    fam = fn.native_family
    return K.kernel_points_grad(tx1, tx2, theta, fam, tU, tV), K.kernel_points_grad(tx2, tx1, theta, fam, tV, tU)


# (family, B, M, N, D, t, ARD, kind, x2 is x1): every padded D (4, 8, 16, 32), a row-block crossing (257), ragged LDS
# tiles (77, 130, 257, 300), the 8-column sweep boundary (t = 9, 17), both lengthscale forms, batching, both orientations of
# a rectangular pair, equal sizes with different tensors, exact r = 0 off the diagonal
POINT_CASES = [
    ("rbf", 1, 1, 1, 1, 1, False, "plain", False),
    ("rbf", 1, 257, 257, 3, 1, True, "plain", True),
    ("matern12", 3, 130, 77, 1, 9, False, "plain", False),
    ("matern32", 1, 77, 130, 8, 4, True, "plain", False),
    ("matern52", 1, 63, 63, 32, 17, False, "plain", True),
    ("matern52", 1, 64, 64, 5, 2, True, "plain", False),
    ("rbf", 1, 64, 64, 2, 3, True, "dup", True),
    ("matern12", 1, 64, 64, 2, 3, True, "dup", True),
    ("matern32", 1, 64, 64, 2, 3, False, "dup", True),
    ("matern52", 1, 64, 64, 2, 3, True, "dup", True),
    ("matern32", 1, 40, 300, 13, 2, True, "plain", False),  # (D padded to 16)
]


def points_check(case, seed):
    name, B, M, N, D, t, ard, kind, same = case
    label = "-".join(str(x) for x in case)
    fn = covariance.FAMILIES[name]
    x1, x2, ls, os_ = make_points(seed, B, M, N, D, ard, kind, same)
    g = rng(seed + 1)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    want1, want2 = autograd_points(fn, x1, x2, ls, os_, U, V, torch.float64)
    ref1, ref2 = autograd_points(fn, x1, x2, ls, os_, U, V, torch.float32)
    tU, tV = dev(U), dev(V)
    # the kernel, both sides
    tx1 = dev(x1)
    tx2 = tx1 if same else dev(x2)
    g1, g2 = native_both_sides(fn, tx1, tx2, ls, os_, tU, tV)
    assert g1.shape == (B, M, D) and g2.shape == (B, N, D)
    within_bound(label + " x1", g1, want1, ref1)
    within_bound(label + " x2", g2, want2, ref2)
    # the operator: points, lengthscale and outputscale all ask for a gradient; nothing is evaluated densely
    lx1 = dev(x1).requires_grad_(True)
    lx2 = lx1 if same else dev(x2).requires_grad_(True)
    tl, to = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    op = KernelLinearOperator(lx1, lx2, never_called(fn), num_nonbatch_dimensions=NB, lengthscale=tl, outputscale=to)
    assert op._same_points() == same
    with no_dense():
        gx1, gx2, gl, go = op._bilinear_derivative(tU, tV)
    assert gx1.shape == lx1.shape and gx2.shape == lx2.shape
    assert torch.equal(gx1, g1) and torch.equal(gx2, g2)
    # lengthscale and outputscale: the bits of lo_kernel_bilinear_f32 under the chain rule, as before
    theta = K.kernel_theta(tl, to, (B,), D)
    gt = K.kernel_bilinear(tx1, tx2, theta, fn.native_family, tU, tV)
    d_ls = (-(theta[:, :D] ** 2) * gt[:, :D]).reshape(B, 1, D)
    if not ard and D > 1:
        d_ls = d_ls.sum(-1, keepdim=True)
    assert gl.shape == tl.shape and torch.equal(gl, d_ls)
    assert go.shape == to.shape and torch.equal(go, 2.0 * to.detach() * gt[:, D])
    # only the points ask: the other two are None and the points' gradients are the same bits
    op = KernelLinearOperator(lx1, lx2, never_called(fn), num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                              outputscale=dev(os_))
    with no_dense():
        hx1, hx2, hl, ho = op._bilinear_derivative(tU, tV)
    assert hl is None and ho is None and torch.equal(hx1, g1) and torch.equal(hx2, g2)


@pytest.mark.parametrize("case", POINT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_points_gradient_against_fp64_autograd(case):
    points_check(case, 7000 + 3 * POINT_CASES.index(case))


def test_one_side_only_and_broadcast_batches():
    """Only x2 asks for a gradient (no call for x1); x2 is shared by the members of the batch: the gradient has the
    leaf's shape, summed over the batch."""
    B, M, N, D, t = 3, 70, 45, 3, 2
    x1, x2, ls, os_ = make_points(7100, B, M, N, D, True)
    x2 = x2[:1]
    g = rng(7101)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    fn = covariance.matern32

    def autograd(dtype):
        b = dev(x2[0], dtype).requires_grad_(True)
        (dev(U, dtype) * (fn(dev(x1, dtype), b, dev(ls, dtype), dev(os_, dtype)) @ dev(V, dtype))).sum().backward()
        return host(b.grad)

    leaf = dev(x2[0]).requires_grad_(True)  # [N, D], broadcast over the batch by the constructor
    op = KernelLinearOperator(dev(x1), leaf, never_called(fn), num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                              outputscale=dev(os_))
    with no_dense(), mock.patch.object(K, "kernel_points_grad", wraps=K.kernel_points_grad) as spy:
        (op @ dev(V)).backward(dev(U))
    assert spy.call_count == 1
    assert leaf.grad.shape == (N, D)
    within_bound("x2 alone, shared by 3 members", leaf.grad, autograd(torch.float64), autograd(torch.float32))


def test_points_gradient_without_a_column_split():
    """B ceil(M / 256) >= 512 workgroups: a thread sweeps all the columns of its row, no partials, no second kernel."""
    case = ("rbf", 512, 40, 40, 2, 2, True, "plain", True)
    assert _hip.load().lo_kernel_points_grad_workspace_bytes(512, 40, 40, 2, 2) == 256  # (nothing but the tail)
    points_check(case, 7200)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_far_points_give_a_finite_zero_gradient(name):
    B, N, D, t = 1, 257, 3, 4
    fn = covariance.FAMILIES[name]
    x1, x2, ls, os_ = make_points(7300, B, N, N, D, True, "far")
    g = rng(7301)
    U, V = g.standard_normal((B, N, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    want1, want2 = autograd_points(fn, x1, x2, ls, os_, U, V, torch.float64)
    assert np.abs(want1).max() <= 1e-12 and np.abs(want2).max() <= 1e-12  # (0 at the scale of float32)
    tx = dev(x1)
    g1, g2 = native_both_sides(fn, tx, tx, ls, os_, dev(U), dev(V))
    for got, want in ((g1, want1), (g2, want2)):
        assert torch.isfinite(got).all()
        print(f"kernel_points_grad {name}-far: max |g| {np.abs(host(got)).max():.3e}")
        assert np.abs(host(got) - want).max() <= ERR_FLOOR


@pytest.mark.parametrize("shape", [(3, 1013, 700, 8, 5), (512, 40, 40, 2, 2)], ids=["split", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, M, N, D, t = shape
    lib = _hip.load()
    assert (lib.lo_kernel_points_grad_workspace_bytes(B, M, N, D, t) > 256) == (shape[1] == 1013)
    x1, x2, ls, os_ = make_points(7400, B, M, N, D, True)
    tx1, tx2 = dev(x1), dev(x2)
    U, V = torch.randn(B, M, t, device=DEV), torch.randn(B, N, t, device=DEV)
    first = native_both_sides(covariance.matern52, tx1, tx2, ls, os_, U, V)
    again = native_both_sides(covariance.matern52, tx1, tx2, ls, os_, U, V)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def test_error_codes_of_the_entry_point():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, t = 1, 300, 300, 3, 2
    x = torch.rand(B, M, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    U, V = torch.randn(B, M, t, device=DEV), torch.randn(B, N, t, device=DEV)
    g = torch.full((B, M, D), -7.0, device=DEV)
    st = _hip.stream_ptr(x.device)
    need = lib.lo_kernel_points_grad_workspace_bytes(B, M, N, D, t)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def pg(x1=x, xb=x, th=theta, fam=0, b=B, m=M, n=N, dim=D, uu=U, vv=V, tt=t, gg=g, w=ws, wb=need):
        return lib.lo_kernel_points_grad_f32(p(x1), p(xb), p(th), fam, b, m, n, dim, p(uu), p(vv), tt, p(gg), p(w), wb, st)

    for bad in (dict(gg=None), dict(fam=4), dict(x1=None), dict(xb=None), dict(th=None), dict(uu=None), dict(vv=None),
                dict(fam=-1), dict(b=0), dict(m=0), dict(n=-1), dict(dim=0), dict(tt=0)):
        assert pg(**bad) == -1, bad  # LO_ERR_BADARG
    assert pg(dim=33) == _hip.LO_ERR_UNSUPPORTED
    assert pg(wb=need - 1) == -3 and pg(w=None, wb=0) == -3  # LO_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())  # (none of them launched anything)
    assert pg() == 0
    torch.cuda.synchronize()
    assert torch.equal(g, K.kernel_points_grad(x, x, theta, 0, U, V))
    with pytest.raises(RuntimeError, match="kernel_points_grad"):
        K.kernel_points_grad(x, x[:, :-1], theta, 0, U, V)


def test_points_gradient_never_holds_the_matrix():
    """N = 32768: a dense K would be 4 GiB and the differences of one autograd row block 64 MiB; both gradients together
    may allocate 64 N (D + t) floats (the workspace is 4 partial copies of [N, D], the two results are [N, D] each)."""
    N, D, t = 32768, 4, 1
    g = torch.Generator().manual_seed(7500)
    x = torch.rand(N, D, generator=g).to(DEV).requires_grad_(True)
    ls, os_ = torch.full((1, D), 0.3, device=DEV), torch.tensor(1.2, device=DEV)
    U, V = torch.randn(N, t, generator=g).to(DEV), torch.randn(N, t, generator=g).to(DEV)
    op = KernelLinearOperator(x, x, never_called(covariance.rbf), num_nonbatch_dimensions=NB, lengthscale=ls,
                              outputscale=os_)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with no_dense():
        gx1, gx2, gl, go = op._bilinear_derivative(U, V)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"kernel_points_grad N={N}: peak growth {growth} bytes, allowed {64 * N * (D + t) * 4}")
    assert growth < 64 * N * (D + t) * 4
    assert gx1.shape == x.shape and gx2.shape == x.shape and gl is None and go is None
    a = x.detach()[:8].double().requires_grad_(True)
    (U[:8].double() * (covariance.rbf(a, x.detach().double(), ls.double(), os_.double()) @ V.double())).sum().backward()
    assert rel(host(gx1[:8]), host(a.grad)) <= 1e-5


def test_deep_kernel_learning_step():
    """x = tanh(z W), inv_quad of K(x, x) + D under the solver settings of the golden tests, gradient of W.  The float32
    run of the bound is the same computation on the stored dense K (torch autograd from K to W) under the same settings:
    cg_tolerance is part of the function, for both."""
    n, d_in, D = 300, 6, 3
    g = rng(7600)
    z = g.standard_normal((n, d_in)).astype(np.float32)
    W = (0.5 * g.standard_normal((d_in, D))).astype(np.float32)
    ls = (0.6 + 0.3 * g.random((1, D))).astype(np.float32)
    os_ = np.float32(1.1)
    noise = (0.05 + 0.1 * g.random(n)).astype(np.float32)
    rhs = g.standard_normal((n, 1)).astype(np.float32)
    fn = covariance.matern52

    def leaves(dtype):
        w = dev(W, dtype).requires_grad_(True)
        return w, torch.tanh(dev(z, dtype) @ w)

    w64, x64 = leaves(torch.float64)
    K64 = fn(x64, x64, dev(ls, torch.float64), dev(os_, torch.float64)) + torch.diag_embed(dev(noise, torch.float64))
    (dev(rhs, torch.float64) * torch.linalg.solve(K64, dev(rhs, torch.float64))).sum().backward()
    with solver_settings(settings):
        w32, x32 = leaves(torch.float32)
        dense = DenseLinearOperator(fn(x32, x32, dev(ls), dev(os_)))
        AddedDiagLinearOperator(dense, DiagLinearOperator(dev(noise))).inv_quad(dev(rhs)).sum().backward()
        w, x = leaves(torch.float32)
        op = KernelLinearOperator(x, x, never_called(fn), num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                                  outputscale=dev(os_))
        A = AddedDiagLinearOperator(op, DiagLinearOperator(dev(noise)))
        assert A._kernel_descriptor().kind == _hip.LO_OP_KERNEL_DIAG
        with no_dense():
            A.inv_quad(dev(rhs)).sum().backward()
    within_bound("deep kernel learning, d inv_quad / d W", w.grad, host(w64.grad), host(w32.grad))


def test_inducing_points_step():
    """K(X, Z) rectangular, Z learned: the gradient of sum(K v) through the public product."""
    M, N, D, c = 130, 77, 3, 2
    X, Z, ls, os_ = make_points(7700, 1, M, N, D, True)
    X, Z, ls, os_ = X[0], Z[0], ls[0], os_[0]
    v = rng(7701).standard_normal((N, c)).astype(np.float32)
    fn = covariance.matern32

    def autograd(dtype):
        b = dev(Z, dtype).requires_grad_(True)
        (fn(dev(X, dtype), b, dev(ls, dtype), dev(os_, dtype)) @ dev(v, dtype)).sum().backward()
        return host(b.grad)

    tZ = dev(Z).requires_grad_(True)
    op = KernelLinearOperator(dev(X), tZ, never_called(fn), num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                              outputscale=dev(os_))
    with no_dense():
        (op @ dev(v)).sum().backward()
    assert tZ.grad.shape == (N, D)
    within_bound("inducing points, d sum(K v) / d Z", tZ.grad, autograd(torch.float64), autograd(torch.float32))
