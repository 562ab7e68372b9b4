"""The float64 matrix-free kernel operator on the device (ABI 31, csrc/lo_kernel_op_f64.hip): lo_kernel_mv_f64,
lo_kernel_bilinear_f64, lo_kernel_points_grad_f64 and the float64 kind LO_OP_KERNEL_DIAG of lo_matvec_f64, directly and
behind KernelLinearOperator, AddedDiag and Sum, against the reference's float64 goldens g42
(tests/golden/make_golden_kernel_f64.py).

Bounds.  The truth is the numpy longdouble computation of tests/kernel_f64_cases.py on the same float64 inputs (tested
against float64 autograd in tests/test_kernel_f64_cpu.py).  `ref_err` is the error of the torch float64 composition on the
device -- covariance.f(x1, x2, ls, os) @ v, float64 autograd through it for the derivatives -- and the native error must
be <= REF_FACTOR = 4 times max(ref_err, 2^-52).  Every test prints the ratio it measured.  Golden quantities: the error
against the fixture's exact value is at most 4 times max(the reference's own recorded error, 2^-52)."""
import ctypes
import os
import sys
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import kernel_f64_cases as T  # noqa: E402
from kernel_f64_cases import FLOOR, REF_FACTOR, rel  # noqa: E402
from make_golden_kernel_f64 import CASES, CG_TOLERANCE, PROBES, RANK, inputs  # noqa: E402
from make_golden_kernel_op import solver_settings  # noqa: E402

pytestmark = pytest.mark.gpu

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, RootLinearOperator)
from linear_operator_amd.operators.added_diag_linear_operator import clear_preconditioner_memo  # noqa: E402

DEV = "cuda"
NB = {"outputscale": 0}
NAMES = list(covariance.FAMILIES)
F64 = torch.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def within_bound(label, native, truth, ref):
    err, ref_err = rel(host(native), truth), max(rel(host(ref), truth), FLOOR)
    print(f"kernel_f64 {label}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert np.isfinite(host(native)).all(), label
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def problem(seed, B, M, N, D, ard, same=False):
    """(x1, x2, ls, os) in float64 numpy; `same`: x2 is x1."""
    g = rng(seed)
    x1 = g.random((B, M, D))
    x2 = x1 if same else g.random((B, N, D))
    ls = 0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))
    os_ = 0.8 + 0.7 * g.random(B)
    return x1, x2, ls, os_


def theta_of(ls, os_, B, D):
    return K.kernel_theta(dev(ls), dev(os_), (B,), D, dtype=F64)


def diag_of(mode, B, N, seed):
    if mode == "none":
        return None, None, False
    if mode == "full":
        d = 0.5 + rng(seed).random((B, N))
        return d[:, :, None], dev(d), False
    d = 0.5 + rng(seed).random(B)
    return d[:, None, None], dev(d), True


def kernel_op(name, x1, x2, ls, os_, fn=None):
    return KernelLinearOperator(x1, x2, fn or covariance.FAMILIES[name], num_nonbatch_dimensions=NB, lengthscale=ls,
                                outputscale=os_)


# ---------------------------------------------------------------------------------- products
def check_mv(name, B, M, N, D, c, mode, ard, seed):
    same = M == N
    x1, x2, ls, os_ = problem(seed, B, M, N, D, ard, same)
    v = rng(seed + 1).standard_normal((B, N, c))
    dn, dt, const = diag_of(mode if same else "none", B, N, seed + 2)
    theta = theta_of(ls, os_, B, D)
    truth = T.dense_ld(name, x1, x2, host(theta)) @ v.astype(T.LD)
    t1, t2, tv, tl, to = dev(x1), dev(x2), dev(v), dev(ls), dev(os_)
    t2 = t1 if same else t2
    ref = covariance.FAMILIES[name](t1, t2, tl, to) @ tv
    if dn is not None:
        truth = truth + dn.astype(T.LD) * v
        ref = ref + dev(np.broadcast_to(dn, (B, N, 1)).copy()) * tv
    y = K.kernel_mv(t1, t2, theta, T.FAMILY_CODES[name], tv, dt, const)
    assert y.dtype == F64 and tuple(y.shape) == (B, M, c)
    label = f"mv {name} B{B} M{M} N{N} D{D} c{c} {mode} {'ard' if ard else 'shared'}"
    within_bound(label, y, truth, ref)
    assert torch.equal(y, K.kernel_mv(t1, t2, theta, T.FAMILY_CODES[name], tv, dt, const)), "two calls differ"
    op = kernel_op(name, t1, t2, tl, to)
    assert op._is_native_f64()
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        ym = op._matmul(tv)
    plain = y if dt is None else K.kernel_mv(t1, t2, theta, T.FAMILY_CODES[name], tv)
    assert torch.equal(ym, plain), "the operator's _matmul is not lo_kernel_mv_f64"


@pytest.mark.parametrize("D", [1, 3, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("name", NAMES)
def test_every_family_meets_every_padded_dimension(name, D):
    check_mv(name, 1, 63, 63, D, 5, "full", D % 2 == 1, 7000 + D)


@pytest.mark.parametrize("name,B,N,D,c,mode,ard", [
    ("rbf", 1, 1, 1, 1, "none", False),          # one thread
    ("matern12", 3, 63, 3, 4, "full", True),     # a ragged tile
    ("matern32", 1, 63, 4, 33, "const", False),
    ("matern52", 3, 257, 5, 17, "full", True),   # two tiles and a row block boundary
    ("rbf", 1, 257, 8, 1, "none", True),
    ("matern12", 1, 257, 9, 33, "const", False),
    ("matern32", 3, 257, 16, 4, "full", True),
    ("matern52", 1, 257, 17, 5, "const", True),
    ("rbf", 1, 257, 32, 17, "full", True),
    ("matern52", 1, 1013, 3, 33, "full", True),  # eight tiles with the column split
    ("matern12", 1, 1013, 32, 1, "none", False),
    ("matern32", 3, 1013, 8, 5, "const", True),
    ("rbf", 512, 130, 1, 1, "full", False),      # unsplit, two tiles: ko_shape gives js = 1
])
def test_products_over_the_branches(name, B, N, D, c, mode, ard):
    check_mv(name, B, N, N, D, c, mode, ard, 7100 + N + D + c)


@pytest.mark.parametrize("c", [1, 4, 5, 17, 33])
@pytest.mark.parametrize("D", [3, 32])
def test_both_sides_of_every_column_chunk(D, c):
    check_mv("matern52", 3, 257, 257, D, c, "none", True, 7200 + D + c)


@pytest.mark.parametrize("M,N", [(130, 77), (77, 130)])
@pytest.mark.parametrize("name", NAMES)
def test_rectangular_products_and_the_transpose(name, M, N):
    check_mv(name, 3, M, N, 3, 4, "none", True, 7300 + M)
    x1, x2, ls, os_ = problem(7300 + M, 3, M, N, 3, True)
    op = kernel_op(name, dev(x1), dev(x2), dev(ls), dev(os_))
    w = dev(rng(7301).standard_normal((3, M, 2)))
    theta = theta_of(ls, os_, 3, 3)
    assert torch.equal(op._t_matmul(w), K.kernel_mv(dev(x2), dev(x1), theta, T.FAMILY_CODES[name], w))


@pytest.mark.parametrize("name", NAMES)
def test_duplicated_far_and_overflowing_points(name):
    fam = T.FAMILY_CODES[name]
    # duplicated points: r = 0 off the diagonal
    x1, _, ls, os_ = problem(7400, 2, 130, 130, 3, True, same=True)
    x1[:, 1::2] = x1[:, 0::2]
    v = rng(7401).standard_normal((2, 130, 4))
    theta = theta_of(ls, os_, 2, 3)
    t1 = dev(x1)
    y = K.kernel_mv(t1, t1, theta, fam, dev(v))
    within_bound(f"mv {name} duplicated points", y, T.dense_ld(name, x1, x1, host(theta)) @ v.astype(T.LD),
                 covariance.FAMILIES[name](t1, t1, dev(ls), dev(os_)) @ dev(v))
    # far points: K is outputscale^2 I to 1e-14
    far = np.arange(130, dtype=np.float64)[None, :, None] * np.array([1e3, -1e3, 1e3]) + x1
    dn, dt, _ = diag_of("full", 2, 130, 7402)
    want = os_[:, None, None] ** 2 * v + dn * v
    y = K.kernel_mv(dev(far), dev(far), theta, fam, dev(v), dt)
    assert rel(host(y), want) <= 1e-14
    # coordinates +-1e160: r^2 overflows; every family is finite and equal to os^2 v + d o v (the torch composition
    # gives NaN for the Matern families there: it is not the comparison)
    huge = np.where(rng(7403).random((2, 130, 3)) < 0.5, -1e160, 1e160)
    huge[:, :, 0] = np.arange(130)[None, :] * 1e160  # (all points distinct)
    y = K.kernel_mv(dev(huge), dev(huge), theta, fam, dev(v), dt)
    assert np.isfinite(host(y)).all() and rel(host(y), want) <= 1e-14, name


def test_two_calls_give_equal_bits_and_a_canary_behind_y_survives():
    lib = _hip.load()
    for B, N, D in ((1, 1013, 8), (512, 130, 1)):  # split and unsplit
        x1, _, ls, os_ = problem(7500 + N, B, N, N, D, True, same=True)
        v = dev(rng(7501).standard_normal((B, N, 33)))
        theta, t1 = theta_of(ls, os_, B, D), dev(x1)
        assert torch.equal(K.kernel_mv(t1, t1, theta, 3, v), K.kernel_mv(t1, t1, theta, 3, v))
    B, N, D, c = 1, 1013, 8, 33
    x1, _, ls, os_ = problem(7510, B, N, N, D, True, same=True)
    v = dev(rng(7511).standard_normal((B, N, c)))
    theta, t1 = theta_of(ls, os_, B, D), dev(x1)
    assert tuple(t1.shape) == (B, N, D) and tuple(theta.shape) == (B, D + 1) and tuple(v.shape) == (B, N, c)
    buf = torch.full((B * N * c + 64,), -7.0, dtype=F64, device=DEV)
    need = lib.lo_kernel_mv_f64_workspace_bytes(B, N, N, D, c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.lo_kernel_mv_f64(_hip.ptr(t1), _hip.ptr(t1), _hip.ptr(theta), 3, B, N, N, D, _hip.ptr(v), c, None, 0,
                              _hip.ptr(buf), _hip.ptr(ws), need, _hip.stream_ptr(v.device))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[: B * N * c].view(B, N, c), K.kernel_mv(t1, t1, theta, 3, v))
    assert bool((buf[B * N * c:] == -7.0).all()), "the canary behind y was overwritten"
    # a workspace one byte short, and y == v: refused before any launch
    buf.fill_(-7.0)
    args = (_hip.ptr(t1), _hip.ptr(t1), _hip.ptr(theta), 3, B, N, N, D, _hip.ptr(v), c, None, 0)
    assert lib.lo_kernel_mv_f64(*args, _hip.ptr(buf), _hip.ptr(ws), need - 1, _hip.stream_ptr(v.device)) == -3
    assert lib.lo_kernel_mv_f64(*args, _hip.ptr(v), _hip.ptr(ws), need, _hip.stream_ptr(v.device)) == -1
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    with pytest.raises(_hip.HipExtensionError):  # mixed element types
        K.kernel_mv(t1, t1, theta.float(), 3, v)


# ---------------------------------------------------------------------------------- the descriptor kind
def test_descriptor_product_equals_kernel_mv_bit_for_bit():
    B, N, D, c = 3, 257, 5, 5
    x1, _, ls, os_ = problem(7600, B, N, N, D, True, same=True)
    theta, t1, v = theta_of(ls, os_, B, D), dev(x1), dev(rng(7601).standard_normal((B, N, c)))
    for mode in ("none", "full", "const"):
        _, dt, const = diag_of(mode, B, N, 7602)
        desc = K.kernel_diag_descriptor(t1, theta, 2, dt, const, dtype=F64)
        assert desc.kind == _hip.LO_OP_KERNEL_DIAG and desc.dtype == F64 and desc.R == D and desc.n2 == 2
        assert torch.equal(K.matvec(desc, v), K.kernel_mv(t1, t1, theta, 2, v, dt, const)), mode
        for call in (lambda: K.matvec(desc, v.float()), lambda: K.cg_solve(desc, v.float()),
                     lambda: K.pivoted_cholesky(desc, 5), lambda: desc.c_struct()):
            with pytest.raises(_hip.HipExtensionError):  # a float64 kernel descriptor at an fp32 entry point
                call()
    with pytest.raises(_hip.HipExtensionError):
        K.kernel_diag_descriptor(t1, theta.float(), 2, dtype=F64)


@pytest.mark.parametrize("with_diag", [False, True])
@pytest.mark.parametrize("order", ["kernel,lowrank", "lowrank,kernel", "kernel,kernel,dense"])
def test_sum_descriptors_with_kernel_terms(order, with_diag):
    B, N, D, R = 2, 257, 3, 6
    x1, _, ls, os_ = problem(7700, B, N, N, D, True, same=True)
    _, _, ls2, os2 = problem(7701, B, N, N, D, False, same=True)
    Cn = rng(7702).standard_normal((B, N, R)) / np.sqrt(R)
    An = rng(7703).standard_normal((B, N, N)) / np.sqrt(N)
    t1, th1, th2 = dev(x1), theta_of(ls, os_, B, D), theta_of(ls2, os2, B, D)
    for c in (1, 5):
        v = rng(7704 + c).standard_normal((B, N, c))
        tv = dev(v)
        terms, truth, ref = [], 0, 0
        kernels = iter((("rbf", th1, ls, os_), ("matern52", th2, ls2, os2)))
        for kind in order.split(","):
            if kind == "kernel":
                name, th, l_, o_ = next(kernels)
                terms.append(K.kernel_diag_descriptor(t1, th, T.FAMILY_CODES[name], dtype=F64))
                truth = truth + T.dense_ld(name, x1, x1, host(th)) @ v.astype(T.LD)
                ref = ref + covariance.FAMILIES[name](t1, t1, dev(l_), dev(o_)) @ tv
            elif kind == "lowrank":
                terms.append(K.lowrank_diag_descriptor(dev(Cn), None, dtype=F64))
                truth = truth + Cn.astype(T.LD) @ (Cn.astype(T.LD).swapaxes(-1, -2) @ v.astype(T.LD))
                ref = ref + dev(Cn) @ (dev(Cn).mT @ tv)
            else:
                terms.append(K.dense_diag_descriptor(dev(An), None, dtype=F64))
                truth = truth + An.astype(T.LD) @ v.astype(T.LD)
                ref = ref + dev(An) @ tv
        dn, dt, const = diag_of("full" if with_diag else "none", B, N, 7705)
        if dn is not None:
            truth = truth + dn * v
            ref = ref + dev(np.broadcast_to(dn, (B, N, 1)).copy()) * tv
        desc = K.sum_descriptor(terms, dt, const, dtype=F64)
        y = K.matvec(desc, tv)
        within_bound(f"sum {order} diag {with_diag} c{c}", y, truth, ref)
        assert torch.equal(y, K.matvec(desc, tv))


def test_refusals_launch_nothing_and_the_other_kernel_kinds_stay_refused():
    lib = _hip.load()
    B, N, D, c = 1, 300, 3, 2
    x = torch.rand(B, N, D, dtype=F64, device=DEV)
    theta = torch.ones(B, D + 1, dtype=F64, device=DEV)
    v, y = torch.randn(B, N, c, dtype=F64, device=DEV), torch.full((B, N, c), -7.0, dtype=F64, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_diag_descriptor(x, theta, 0, dtype=F64)
    root = K.lowrank_diag_descriptor(torch.rand(B, N, 4, dtype=F64, device=DEV), None, dtype=F64)
    s = desc.c_struct(F64)
    need = lib.lo_matvec_f64_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda s_: lib.lo_matvec_f64(ctypes.byref(s_), _hip.ptr(v), _hip.ptr(y), c, _hip.ptr(ws), need, st)  # noqa: E731
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        for field, val, rc in (("A0", None, -1), ("A1", None, -1), ("n2", 4, -1), ("n2", -1, -1), ("R", 0, -1),
                               ("R", 33, _hip.LO_ERR_UNSUPPORTED)):
            s = desc.c_struct(F64)
            setattr(s, field, val)
            assert run(s) == rc, (field, val)
            # the same term in the last position of a sum: refused before the first term is launched
            both = K.sum_descriptor([root, desc], dtype=F64).c_struct(F64)
            setattr(both.terms[1], field, val)
            assert run(both) == rc, ("sum", field, val)
        s = desc.c_struct(F64)
        assert lib.lo_matvec_f64(ctypes.byref(s), _hip.ptr(v), _hip.ptr(y), c, _hip.ptr(ws), 8, st) == -3
        assert lib.lo_matvec_f64(ctypes.byref(s), _hip.ptr(v), _hip.ptr(v), c, _hip.ptr(ws), need, st) == -1
        for kind in (_hip.LO_OP_KERNEL_SUM_DIAG, _hip.LO_OP_KERNEL_KRON_DIAG, _hip.LO_OP_KERNEL_GRAD_DIAG):
            s = desc.c_struct(F64)
            s.kind = kind
            assert run(s) == _hip.LO_ERR_UNSUPPORTED, kind
        L, perm = torch.empty(B, 5, N, dtype=F64, device=DEV), torch.empty(B, N, dtype=torch.int64, device=DEV)
        rank = ctypes.c_int32(0)
        s = desc.c_struct(F64)
        assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, _hip.ptr(L), _hip.ptr(perm), ctypes.byref(rank),
                                           _hip.ptr(ws), need, st) == _hip.LO_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _hip.prof_report() == {}, "a refusal launched a kernel"
    finally:
        _hip.prof_enable(False)
    assert bool((y == -7.0).all())
    assert run(desc.c_struct(F64)) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_mv(x, x, theta, 0, v))


# ---------------------------------------------------------------------------------- derivatives
def autograd_all(name, x1, x2, ls, os_, U, V, same):
    a = dev(x1).requires_grad_(True)
    b = a if same else dev(x2).requires_grad_(True)
    l_, o_ = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    (dev(U) * (covariance.FAMILIES[name](a, b, l_, o_) @ dev(V))).sum().backward()
    return a.grad, None if same else b.grad, l_.grad, o_.grad


@pytest.mark.parametrize("M,N,t,D,ard", [(1, 1, 1, 1, False), (130, 130, 8, 3, True), (257, 257, 11, 8, False),
                                         (130, 77, 11, 17, True), (77, 130, 1, 32, True), (257, 130, 8, 16, False)])
@pytest.mark.parametrize("name", NAMES)
def test_derivatives_against_the_analytic_formulas(name, M, N, t, D, ard):
    B, fam = 2, T.FAMILY_CODES[name]
    x1, x2, ls, os_ = problem(7800 + M + t, B, M, N, D, ard)
    U, V = rng(7801).standard_normal((B, M, t)), rng(7802).standard_normal((B, N, t))
    theta = theta_of(ls, os_, B, D)
    th = host(theta)
    g1_ref, g2_ref, gl_ref, go_ref = autograd_all(name, x1, x2, ls, os_, U, V, False)
    t1, t2, tU, tV = dev(x1), dev(x2), dev(U), dev(V)
    g = K.kernel_bilinear(t1, t2, theta, fam, tU, tV)
    assert g.dtype == F64 and tuple(g.shape) == (B, D + 1)
    d_ls, d_os = T.theta_to_params(th, T.g_theta_ld(name, x1, x2, th, U, V), ard)
    got_ls = -(theta[:, :D] ** 2) * g[:, :D]
    got_ls = (got_ls if ard else got_ls.sum(-1, keepdim=True))[:, None, :]
    label = f"{name} M{M} N{N} t{t} D{D} {'ard' if ard else 'shared'}"
    within_bound("d lengthscale " + label, got_ls, d_ls, gl_ref)
    within_bound("d outputscale " + label, 2 * dev(os_) * g[:, D], d_os, go_ref)
    p1 = K.kernel_points_grad(t1, t2, theta, fam, tU, tV)
    p2 = K.kernel_points_grad(t2, t1, theta, fam, tV, tU)
    within_bound("d x1 " + label, p1, T.g_x1_ld(name, x1, x2, th, U, V), g1_ref)
    within_bound("d x2 " + label, p2, T.g_x1_ld(name, x2, x1, th, V, U), g2_ref)
    assert torch.equal(g, K.kernel_bilinear(t1, t2, theta, fam, tU, tV))
    assert torch.equal(p1, K.kernel_points_grad(t1, t2, theta, fam, tU, tV))
    # behind the operator: one call per side that asks, the same theta -> lengthscale / outputscale mapping
    leaves = [dev(a).requires_grad_(True) for a in (x1, x2, ls, os_)]
    op = kernel_op(name, *leaves)
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        grads = op._bilinear_derivative(tU, tV)
    assert torch.equal(grads[0], p1) and torch.equal(grads[1], p2)
    assert torch.allclose(grads[2], got_ls.reshape(leaves[2].shape), rtol=1e-13, atol=0)
    assert torch.allclose(grads[3], 2 * dev(os_) * g[:, D], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_derivatives_at_duplicated_points(name):
    B, N, D, t, fam = 1, 130, 3, 8, T.FAMILY_CODES[name]
    x1, _, ls, os_ = problem(7900, B, N, N, D, True, same=True)
    x1[:, 1::2] = x1[:, 0::2]
    U, V = rng(7901).standard_normal((B, N, t)), rng(7902).standard_normal((B, N, t))
    theta = theta_of(ls, os_, B, D)
    th, t1 = host(theta), dev(x1)
    g = K.kernel_bilinear(t1, t1, theta, fam, dev(U), dev(V))
    p = K.kernel_points_grad(t1, t1, theta, fam, dev(U), dev(V))
    assert np.isfinite(host(g)).all() and np.isfinite(host(p)).all()
    # the truth leaves the coincident pairs out of the Matern-1/2 sums (r^2 <= 1e-30), as the kernels do
    g_truth, p_truth = T.g_theta_ld(name, x1, x1, th, U, V), T.g_x1_ld(name, x1, x1, th, U, V)
    a = t1.clone().requires_grad_(True)
    l_, o_ = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    (dev(U) * (covariance.FAMILIES[name](a, t1, l_, o_) @ dev(V))).sum().backward()
    d_ls, d_os = T.theta_to_params(th, g_truth, True)
    within_bound(f"d lengthscale {name} duplicated", (-(theta[:, :D] ** 2) * g[:, :D])[:, None, :], d_ls, l_.grad)
    within_bound(f"d x1 {name} duplicated", p, p_truth, a.grad)


# ---------------------------------------------------------------------------------- the public API
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g42_kernel_f64_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in ("x", "lengthscale", "outputscale"):
            t[k].requires_grad_(True)
    return t


def spying(fn, seen):
    """covar_func with its returned shapes recorded; `native_family` stays on the wrapper."""
    def spy(x1, x2, **params):
        out = fn(x1, x2, **params)
        seen.append(tuple(out.shape[-2:]))
        return out

    spy.native_family = fn.native_family
    return spy


@pytest.fixture
def wraps(monkeypatch):
    """Counts the Python closures handed to the library as callbacks (kernels._wrap_closure, a pass-through)."""
    count = [0]
    real = K._wrap_closure

    def counting(*a, **kw):
        count[0] += 1
        return real(*a, **kw)

    monkeypatch.setattr(K, "_wrap_closure", counting)
    return count


def api_calls(p, monkeypatch, shut):
    """The public calls on the float64 AddedDiag(Kernel, Diag) of golden case p.  shut=True: the float64 gate answers a
    refusal, which is the parent commit's route (covar_func densely, a Python closure per product)."""
    family = CASES[p][0]
    seen, iterations, out = [], [], {}
    fn = spying(covariance.FAMILIES[family], seen)
    clear_preconditioner_memo()
    with monkeypatch.context() as mp:
        if shut:
            mp.setattr(KernelLinearOperator, "_native_f64_refusal", lambda self, check_device=True: "shut")
        for name in ("cg_solve_f64", "minres_solve_f64"):
            def recording(*a, _real=getattr(K, name), **kw):
                res = _real(*a, **kw)
                iterations.append(res.iterations)
                return res
            mp.setattr(K, name, recording)

        def added(t, cls=AddedDiagLinearOperator):
            return cls(kernel_op(family, t["x"], t["x"], t["lengthscale"], t["outputscale"], fn), DiagLinearOperator(t["noise"]))

        t = tensors(p)

        class Probed(AddedDiagLinearOperator):
            def _probe_vectors_and_norms(self):
                n = t["Z"].norm(dim=-2, keepdim=True)
                return t["Z"] / n, n

        with solver_settings(settings), settings.cg_tolerance(CG_TOLERANCE), settings.num_trace_samples(PROBES), \
                warnings.catch_warnings():
            warnings.simplefilter("ignore")
            A = added(t)
            out["desc"] = A._kernel_descriptor()
            out["mv"] = A._linear_op._matmul(t["V"])
            out["diag"] = A._linear_op._diagonal()
            out["solve"] = A.solve(t["rhs"])
            g = tensors(p, grad=True)
            iq, ld = added(g, Probed).inv_quad_logdet(g["rhs"], logdet=True)
            (iq.sum() + ld.sum()).backward()
            out["iq"], out["ld"] = iq.detach(), ld.detach()
            g2 = tensors(p, grad=True)
            added(g2).inv_quad(g2["rhs"]).sum().backward()
            out["gl"], out["go"], out["gx"] = g2["lengthscale"].grad, g2["outputscale"].grad, g2["x"].grad
            out["sqrt"] = A.sqrt_inv_matmul(t["rhs"])
            torch.manual_seed(4242)
            R = A.root_decomposition().root.to_dense()
            out["root"] = R @ R.mT
            seen_before_rows = list(seen)
            out["L"], piv = A._linear_op.pivoted_cholesky(RANK, return_pivots=True)
            out["piv"] = piv[..., :RANK]
    clear_preconditioner_memo()
    return out, iterations, seen, seen_before_rows


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_never_forms_the_matrix_and_meets_the_goldens(p, wraps, monkeypatch):
    """Fails without the feature: on the parent commit covar_func returns the [B, N, N] matrix once per product and the
    product is a wrapped Python closure."""
    G = golden(p)
    _, B, N, D, _, _ = CASES[p]
    native, it_native, seen, _ = api_calls(p, monkeypatch, shut=False)
    assert wraps[0] == 0, f"{wraps[0]} Python closures were wrapped for the product or the preconditioner"
    big = [s for s in seen if s[0] > 1 and s[1] > 1]
    assert not big, f"covar_func returned matrices {sorted(set(big))}"
    desc = native.pop("desc")
    assert desc is not None and desc.kind == _hip.LO_OP_KERNEL_DIAG and desc.dtype == F64 and desc.N == N and desc.R == D
    assert all(v.dtype in (F64, torch.int64) for v in native.values())
    # the parent's route: the gate patched shut
    shut, it_shut, seen_shut, _ = api_calls(p, monkeypatch, shut=True)
    assert shut.pop("desc") is None and wraps[0] > 0 and any(s == (N, N) for s in seen_shut)
    assert it_native == it_shut, (it_native, it_shut)
    for key in native:
        if key == "piv":
            assert torch.equal(native[key], shut[key])
            continue
        err = rel(host(native[key]), host(shut[key]))
        print(f"kernel_f64 {p} {key}: native against the closure route {err:.3e}")
        assert native[key].shape == shut[key].shape and err < 1e-9, (key, err)
    # against the goldens
    assert np.array_equal(host(native["piv"]), G["piv"])
    for q in ("mv", "diag", "solve", "iq", "ld", "L", "gl", "go", "gx"):
        err, ref_err = rel(host(native[q]), G[q + "_exact"]), max(float(G[q + "_err"]), FLOOR)
        print(f"kernel_f64 {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
        assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def test_sums_kronecker_and_the_prediction_product(wraps):
    B, N, D = 2, 257, 3
    x1, _, ls, os_ = problem(8000, B, N, N, D, True, same=True)
    _, _, ls2, os2 = problem(8001, B, N, N, D, False, same=True)
    Cn = rng(8002).standard_normal((B, N, 4)) / 2
    noise, rhs = 0.05 + 0.1 * rng(8003).random((B, N)), rng(8004).standard_normal((B, N, 1))
    tx = dev(x1)
    seen = []
    k1 = kernel_op("rbf", tx, tx, dev(ls), dev(os_), spying(covariance.rbf, seen))
    k2 = kernel_op("matern52", tx, tx, dev(ls2), dev(os2), spying(covariance.matern52, seen))
    th1, th2 = host(theta_of(ls, os_, B, D)), host(theta_of(ls2, os2, B, D))
    K1, K2 = T.dense_ld("rbf", x1, x1, th1), T.dense_ld("matern52", x1, x1, th2)
    Dn = np.stack([np.diag(n) for n in noise]).astype(T.LD)
    clear_preconditioner_memo()
    with solver_settings(settings), settings.cg_tolerance(CG_TOLERANCE), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # Kernel + LowRankRoot + Diag
        A = (k1 + RootLinearOperator(dev(Cn))) + DiagLinearOperator(dev(noise))
        desc = A._kernel_descriptor()
        assert desc is not None and desc.kind == _hip.LO_OP_SUM and desc.dtype == F64
        assert [t.kind for t in desc.terms] == [_hip.LO_OP_KERNEL_DIAG, _hip.LO_OP_LOWRANK_DIAG]
        dense = (K1 + Cn.astype(T.LD) @ Cn.astype(T.LD).swapaxes(-1, -2) + Dn).astype(np.float64)
        err = rel(host(A.solve(dev(rhs))), np.linalg.solve(dense, rhs))
        print(f"kernel_f64 Kernel + LowRankRoot + Diag solve: err {err:.3e}")
        assert err <= 4e-6  # (CG stopped at cg_tolerance 1e-6: the bound of the goldens' solve, 4 x 1e-6)
        # Kernel_rbf + Kernel_m52 + Diag: a float64 LO_OP_SUM of two kernel terms, each its own sweep
        S = (k1 + k2) + DiagLinearOperator(dev(noise))
        desc = S._kernel_descriptor()
        assert desc is not None and desc.kind == _hip.LO_OP_SUM and desc.dtype == F64
        assert [t.kind for t in desc.terms] == [_hip.LO_OP_KERNEL_DIAG] * 2 and desc.diag_mode == _hip.LO_DIAG_FULL
        dense = (K1 + K2 + Dn).astype(np.float64)
        err = rel(host(S.solve(dev(rhs))), np.linalg.solve(dense, rhs))
        print(f"kernel_f64 Kernel + Kernel + Diag solve: err {err:.3e}")
        assert err <= 4e-6
        v = rng(8005).standard_normal((B, N, 3))
        within_bound("Kernel + Kernel + Diag matmul", S._matmul(dev(v)), (K1 + K2 + Dn) @ v.astype(T.LD),
                     (covariance.rbf(tx, tx, dev(ls), dev(os_)) + covariance.matern52(tx, tx, dev(ls2), dev(os2))
                      + torch.diag_embed(dev(noise))) @ dev(v))
    assert wraps[0] == 0 and not [s for s in seen if s[0] > 1 and s[1] > 1]
    # Kronecker(Kernel, Dense) keeps the per-factor composition; its kernel factor multiplies natively
    Bt = np.eye(2) + 0.3 * rng(8006).random((B, 2, 2))
    kp = KroneckerProductLinearOperator(k1, DenseLinearOperator(dev(Bt)))
    v = rng(8007).standard_normal((B, 2 * N, 2))
    truth = np.einsum("bij,bjtc->bitc", K1, np.einsum("bts,bjsc->bjtc", Bt.astype(T.LD), v.reshape(B, N, 2, 2).astype(T.LD)))
    ref = torch.kron(covariance.rbf(tx[0], tx[0], dev(ls)[0], dev(os_)[0]), dev(Bt)[0]) @ dev(v)[0]
    y = kp._matmul(dev(v))
    within_bound("Kronecker(Kernel, Dense) matmul", y[0], truth.reshape(B, 2 * N, 2)[0], ref)
    # the prediction product K(x*, X) alpha, rectangular
    xs = rng(8008).random((B, 77, D))
    pred = kernel_op("rbf", dev(xs), tx, dev(ls), dev(os_), spying(covariance.rbf, seen))
    alpha = rng(8009).standard_normal((B, N, 1))
    within_bound("prediction K(x*, X) alpha", pred._matmul(dev(alpha)), T.dense_ld("rbf", xs, x1, th1) @ alpha.astype(T.LD),
                 covariance.rbf(dev(xs), tx, dev(ls), dev(os_)) @ dev(alpha))
    assert not [s for s in seen if s[0] > 1 and s[1] > 1], "covar_func was evaluated densely"
    # a float32 right-hand side against the float64 operator stays on the general path
    seen.clear()
    with pytest.raises(RuntimeError):
        pred._matmul(dev(alpha).float())
    assert seen == [(77, N)]


def test_memory_at_n_8192():
    """The stored float64 K would be 512 MiB: the product and a solve's products allocate less than 16 MiB."""
    N, D = 8192, 3
    x1, _, ls, os_ = problem(8100, 1, N, N, D, True, same=True)
    tx, v = dev(x1[0]), dev(rng(8101).standard_normal((N, 1)))
    op = kernel_op("matern52", tx, tx, dev(ls[0]), torch.tensor(float(os_[0]), dtype=F64, device=DEV))
    assert op._is_native_f64()
    A = AddedDiagLinearOperator(op, DiagLinearOperator(dev(0.05 + 0.1 * rng(8102).random(N))))
    clear_preconditioner_memo()
    with settings.max_cholesky_size(0), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        op._matmul(v), A.solve(v)  # (warm the allocator's workspaces and the preconditioner)
        torch.cuda.synchronize()
        for label, call in (("_matmul", lambda: op._matmul(v)), ("solve", lambda: A.solve(v))):
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            call()
            torch.cuda.synchronize()
            grown = torch.cuda.max_memory_allocated() - before
            print(f"kernel_f64 memory {label} at N {N}: {grown / 2 ** 20:.2f} MiB")
            assert grown < 16 * 2 ** 20, (label, grown)
    clear_preconditioner_memo()
