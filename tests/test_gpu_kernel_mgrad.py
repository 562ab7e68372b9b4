"""The matrix-free Matern-5/2 gradient kernel (csrc/lo_kernel_mgrad.hip, LO_OP_KERNEL_MGRAD_DIAG) on the MI355X against
the float64 dense matrix of covariance.matern52_grad.  Bounds: the rule of tests/test_gpu_kernel_grad.py -- the error
against float64 is at most REF_FACTOR = 4 times the error of the float32 dense composition of the same computation on the
same inputs (floored at ERR_FLOOR = 1e-7).  Every test prints the ratio it measured."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

from make_golden_kernel_op import ERR_FLOOR, pivot_gaps, rel, solver_settings  # noqa: E402
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
FN = covariance.matern52_grad


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_mgrad {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def make_inputs(seed, B, M, N, D, c, ard=True, dup=False):
    """Points (x2 is x1 when M == N), hyperparameters, columns and a full diagonal that differs per row."""
    g = rng(seed)
    x1 = g.random((B, M, D)).astype(np.float32)
    if dup:  # every other point repeats its neighbour: pairs with u = 0 off the diagonal
        x1[:, 1::2] = x1[:, : x1[:, 1::2].shape[1] * 2: 2]
    x2 = x1 if M == N else g.random((B, N, D)).astype(np.float32)
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    v = g.standard_normal((B, N * (D + 1), c)).astype(np.float32)
    d = (0.05 + g.random((B, M * (D + 1)))).astype(np.float32)
    return x1, x2, ls, os_, v, d


def operator(x1, x2, ls, os_, func=None):
    return KernelLinearOperator(x1, x2, func or FN, num_outputs_per_input=(x1.shape[-1] + 1,) * 2,
                                num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)


# (B, M, N, D, c, diagonal, duplicated points).  The j tile holds 128 points, a row block 256 rows: n of 1, 127, 129, 257.
# D of 1, 3 / 5 / 16: every padded width, whose column chunks are 4 / 2 / 1, so c of 1, chunk + 1 and 17.  N <= 128 and
# B = 512 are not split over j; 3 x 700 is the few-rows / many-columns shape (6 splits); 129 x 257 is rectangular.
MV_CASES = [(1, 1, 1, 1, 1, "none", False), (1, 127, 127, 3, 5, "full", False), (3, 129, 129, 5, 3, "const", False),
            (1, 257, 257, 16, 2, "full", False), (1, 257, 257, 3, 17, "none", True), (3, 257, 257, 1, 1, "full", False),
            (1, 129, 257, 5, 17, "none", False), (1, 3, 700, 3, 1, "none", False), (1, 127, 127, 16, 17, "const", True),
            (512, 40, 40, 2, 2, "full", False)]


@pytest.mark.parametrize("case", MV_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_product_against_the_fp64_dense_matrix(case):
    B, M, N, D, c, diag, dup = case
    i = MV_CASES.index(case)
    x1, x2, ls, os_, v, d = make_inputs(4200 + i, B, M, N, D, c, ard=i % 2 == 0, dup=dup)
    assert (_hip.load().lo_kernel_mgrad_mv_workspace_bytes(B, M, N, D, c) == 256) == (B == 512 or N <= 128)  # (no split)
    dd = {"none": None, "full": d, "const": d[:, :1]}[diag]

    def composition(dtype):
        y = FN(dev(x1, dtype), dev(x2, dtype), dev(ls, dtype), dev(os_, dtype)) @ dev(v, dtype)
        return host(y if dd is None else y + dev(dd, dtype)[:, :, None] * dev(v, dtype))

    want, comp = composition(torch.float64), composition(torch.float32)
    theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
    tx1 = dev(x1)
    tx2 = tx1 if x2 is x1 else dev(x2)
    td = None if dd is None else dev(dd if diag == "full" else dd[:, 0])
    y = K.kernel_mgrad_mv(tx1, tx2, theta, dev(v), td, const_diag=diag == "const")
    assert y.shape == (B, M * (D + 1), c) and torch.isfinite(y).all()
    within("mv " + "-".join(str(a) for a in case), rel(host(y), want), rel(comp, want))
    assert torch.equal(y, K.kernel_mgrad_mv(tx1, tx2, theta, dev(v), td, const_diag=diag == "const"))  # (equal bits per call)
    S = operator(tx1, tx2, dev(ls), dev(os_))
    if diag == "none":  # the operator's product arm, rectangular included
        assert S._native_mgrad_refusal() is None and torch.equal(S._matmul(dev(v)).reshape(y.shape), y)
    if M == N:  # the kind through lo_matvec_f32 runs the same kernel: the same bits
        desc = K.kernel_mgrad_diag_descriptor(tx1, theta, td, const_diag=diag == "const")
        assert desc.kind == S._kernel_descriptor().kind == _hip.LO_OP_KERNEL_MGRAD_DIAG and desc.N == M * (D + 1)
        assert torch.equal(K.matvec(desc, dev(v)), y)


# (B, M, N, D, t, ARD, duplicated points): the same edges of n and D; the derivative's column chunks are 8 / 4 / 2, so t of
# 1 and chunk + 1; the duplicated points reach the branch that drops g3
BIL_CASES = [(1, 1, 1, 1, 1, True, False), (1, 127, 127, 3, 9, False, False), (3, 129, 129, 5, 5, True, False),
             (1, 257, 257, 16, 3, True, False), (1, 257, 257, 3, 1, True, True), (1, 129, 257, 5, 1, False, False),
             (1, 127, 127, 16, 3, False, True), (512, 40, 40, 2, 2, True, False)]


@pytest.mark.parametrize("case", BIL_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_bilinear_derivative_against_fp64_autograd(case):
    B, M, N, D, t, ard, dup = case
    x1, x2, ls, os_, V, _ = make_inputs(4300 + BIL_CASES.index(case), B, M, N, D, t, ard=ard, dup=dup)
    U = rng(4399).standard_normal((B, M * (D + 1), t)).astype(np.float32)

    def dense_grads(dtype):
        l, o = dev(ls, dtype).requires_grad_(True), dev(os_, dtype).requires_grad_(True)
        (dev(U, dtype) * (FN(dev(x1, dtype), dev(x2, dtype), l, o) @ dev(V, dtype))).sum().backward()
        return host(l.grad), host(o.grad)

    want, comp = dense_grads(torch.float64), dense_grads(torch.float32)
    tx1 = dev(x1)
    tl, to = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    S = operator(tx1, tx1 if x2 is x1 else dev(x2), tl, to)
    by_name = dict(zip(["x1", "x2"] + list(S._differentiable_kwargs), S._bilinear_derivative(dev(U), dev(V))))
    assert by_name["x1"] is None and by_name["x2"] is None and by_name["lengthscale"].shape == tl.shape
    for k, name in enumerate(("lengthscale", "outputscale")):
        within(f"bilinear {case} {name}", rel(host(by_name[name]), want[k]), rel(comp[k], want[k]))


def dense_pivoted_cholesky(A, rank):
    """The greedy pivoted Cholesky on the dense A [N, N] in A's dtype (ties keep the earlier position): rows [rank, N]."""
    diag, perm, L = A.diagonal().clone(), torch.arange(A.shape[0]), torch.zeros(rank, A.shape[0], dtype=A.dtype)
    for m in range(rank):
        j = m + int(torch.argmax(diag[perm[m:]]))
        perm[[m, j]] = perm[[j, m]]
        piv, others = perm[m], perm[m + 1:]
        L[m, piv] = diag[piv].sqrt()
        L[m, others] = (A[piv, others] - L[:m, piv] @ L[:m, others]) / L[m, piv]
        diag[others] -= L[m, others] ** 2
    return L, perm[:rank]


def test_pivoted_cholesky_rows_and_pivots():
    n, D, rank = 40, 2, 5
    x, _, ls, os_, _, _ = make_inputs(4402, 1, n, n, D, 1)
    A64 = FN(*(torch.from_numpy(a).double() for a in (x, x, ls, os_)))[0]
    # (the first pivot is an exact tie among the points -- equal diagonal entries, the earlier row wins; from then on the
    # float64 lead of every pivot is a thousand float32 roundings or more, so no rounding of the device's turns one)
    assert min(pivot_gaps(A64.numpy(), rank)[1][1:]) > 1e-4
    L64, piv64 = dense_pivoted_cholesky(A64, rank)
    L32, _ = dense_pivoted_cholesky(FN(*(torch.from_numpy(a) for a in (x, x, ls, os_)))[0], rank)
    L, piv = operator(dev(x), dev(x), dev(ls), dev(os_)).pivoted_cholesky(rank, return_pivots=True)
    assert np.array_equal(piv[0, :rank].cpu().numpy(), piv64.numpy())
    within("pivoted Cholesky rows", rel(host(L[0].mT), L64.numpy()), rel(L32.numpy(), L64.numpy()))


def test_solve_and_inv_quad_logdet_with_backward_call_no_dense_function(monkeypatch):
    """(the stochastic logdet and its gradients: bounded by the float32 run on the STORED operator with the same probes)"""
    n, D, c, PROBES = 50, 3, 2, 32  # N = 200
    x, _, ls, os_, rhs, noise = make_inputs(4500, 1, n, n, D, c)
    noise = 0.05 + 0.2 * noise
    calls = []

    def counted(*args, **kwargs):
        calls.append(1)
        return FN(*args, **kwargs)

    counted.native_outputs = "mgrad"
    monkeypatch.setattr(covariance, "matern52_grad", counted)

    def run(dtype, route):
        tl, to = dev(ls, dtype).requires_grad_(True), dev(os_, dtype).requires_grad_(True)
        tx, tn, tr = dev(x, dtype), dev(noise, dtype), dev(rhs, dtype)
        if route == "exact":
            A = FN(tx, tx, tl, to) + torch.diag_embed(tn)
            sol = torch.linalg.solve(A, tr)
            iq, ld = (tr * sol).sum(-2).sum(-1), torch.linalg.slogdet(A)[1]
        else:
            base = (operator(tx, tx, tl, to, covariance.matern52_grad) if route == "native"
                    else DenseLinearOperator(FN(tx, tx, tl, to)))
            A = AddedDiagLinearOperator(base, DiagLinearOperator(tn))
            torch.manual_seed(4501)  # (both routes draw the same probes for the log-determinant)
            with solver_settings(settings), settings.num_trace_samples(PROBES):
                sol = A.solve(tr)
                iq, ld = A.inv_quad_logdet(tr, logdet=True)
        (iq.sum() + ld.sum()).backward()
        return [host(a) for a in (sol, iq, ld, tl.grad, to.grad)]

    got = run(torch.float32, "native")
    assert calls == []
    want, comp = run(torch.float64, "exact"), run(torch.float32, "stored")
    for name, g, w, r in zip(("solve", "inv_quad", "logdet", "d lengthscale", "d outputscale"), got, want, comp):
        within(name, rel(g, w), rel(r, w))


def test_refusals_launch_nothing():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, c = 1, 300, 3, 2
    N = n * (D + 1)
    x, theta = torch.rand(B, n, D, device=DEV), torch.ones(B, D + 1, device=DEV)
    v, y, g = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV), torch.full((B, D + 1), -7.0, device=DEV)
    wide, th17, v180 = torch.rand(1, 10, 17, device=DEV), torch.ones(1, 18, device=DEV), torch.randn(1, 180, 1, device=DEV)
    st = _hip.stream_ptr(v.device)
    need, bneed = lib.lo_kernel_mgrad_mv_workspace_bytes(B, n, n, D, c), lib.lo_kernel_mgrad_bilinear_workspace_bytes(B, n, n, D, c)
    ws = torch.empty(max(need, bneed), dtype=torch.uint8, device=DEV)
    desc = K.kernel_mgrad_diag_descriptor(x, theta)
    both = K.sum_descriptor([desc, K.lowrank_diag_descriptor(torch.rand(B, N, 4, device=DEV), None)]).c_struct()
    sneed = lib.lo_matvec_workspace_bytes(ctypes.byref(desc.c_struct()), c) + need
    sws = torch.empty(sneed, dtype=torch.uint8, device=DEV)

    def mv(xa=x, th=theta, m=n, dim=D, vec=v, cols=c, out=y, w=ws, wb=need):
        return lib.lo_kernel_mgrad_mv_f32(p(xa), p(xa), p(th), B, m, m, dim, p(vec), cols, None, 0, p(out), p(w), wb, st)

    def bil(xa=x, th=theta, m=n, dim=D, vec=v, cols=c, out=g, w=ws, wb=bneed):
        return lib.lo_kernel_mgrad_bilinear_f32(p(xa), p(xa), p(th), B, m, m, dim, p(vec), p(vec), cols, p(out), p(w), wb, st)

    def kind(**fields):
        s = desc.c_struct()
        for name, val in fields.items():
            setattr(s, name, val)
        return lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(sws), sneed, st)

    assert need > 256  # (a split member: partials)
    _hip.prof_enable(True)
    _hip.prof_report()
    try:
        for bad in (dict(xa=None), dict(th=None), dict(vec=None), dict(out=None), dict(m=0), dict(dim=0), dict(cols=0)):
            assert mv(**bad) == -1 and bil(**bad) == -1, bad  # LO_ERR_BADARG
        d17 = dict(xa=wide, th=th17, m=10, dim=17, vec=v180, cols=1)
        assert mv(**d17) == bil(**d17) == _hip.LO_ERR_UNSUPPORTED and lib.lo_kernel_mgrad_mv_workspace_bytes(1, 10, 10, 17, 1) == 0
        assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3 and bil(wb=bneed - 1) == -3 and bil(w=None, wb=0) == -3
        assert kind(A0=None) == -1 and kind(A1=None) == -1 and kind(R=0) == -1 and kind(N=N + 1) == -1
        assert kind(R=17, N=180) == _hip.LO_ERR_UNSUPPORTED
        assert lib.lo_matvec_f32(ctypes.byref(desc.c_struct()), p(v), p(y), c, p(sws), 255, st) == -3
        assert lib.lo_matvec_f32(ctypes.byref(both), p(v), p(y), c, p(sws), sneed, st) == -1  # (not a term of a sum)
        assert K.kernel_mgrad_diag_descriptor(wide, th17) is None
        torch.cuda.synchronize()
        assert _hip.prof_report() == {}
    finally:
        _hip.prof_enable(False)
    assert bool((y == -7.0).all()) and bool((g == -7.0).all())
    assert kind() == 0 and mv() == 0 and bil() == 0  # (the same calls with nothing wrong run)
    torch.cuda.synchronize()
