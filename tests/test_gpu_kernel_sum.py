"""Sums of KernelLinearOperators on the MI355X: lo_kernel_sum_mv_f32 / lo_kernel_sum_bilinear_f32 /
lo_kernel_sum_points_grad_f32 (csrc/lo_kernel_sum.hip) against fp64 numpy and fp64 autograd, the kind
LO_OP_KERNEL_SUM_DIAG and kernel terms of LO_OP_SUM through the public API (solve, inv_quad_logdet, pivoted Cholesky,
gradients) against the reference's goldens (tests/golden/g39_kernel_sum_*.npz).

Bounds: the protocol of tests/test_gpu_kernel_op.py.  Golden quantities: the error against the fixture's float64 value is
at most REF_FACTOR = 4 times the reference's own recorded float32 error (floored at ERR_FLOOR = 1e-7).  Products and
gradients without a golden: 4 times the error of the torch float32 composition (the sum of the dense covariance functions,
autograd through it) measured on the same inputs inside the test, same floor.  Every test prints the ratio it measured
(DESIGN.md section 6m holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_sum import CASES, ERR_FLOOR, PROBES, RANK, inputs, rel, solver_settings  # noqa: E402
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, KernelLinearOperator,
    LowRankRootLinearOperator, SumLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
FAMILY_NAMES = ["rbf", "matern12", "matern32", "matern52"]
REF_ORDERS = 8  # orderings of the points over which the float32 reference's error of a hyperparameter gradient is measured


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def make_points(seed, B, M, N, D, T, ard, kind="plain"):
    """x1 [B, M, D], x2 (x1 itself when M == N), and per term a lengthscale (term t at (t + 1) / 2 of the base scale: short
    and long scales side by side) and an outputscale."""
    g = rng(seed)
    x1 = g.random((B, M, D)).astype(np.float32)
    x2 = x1 if M == N else g.random((B, N, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with r = 0 off the diagonal
        x1 = x1.copy()
        x1[:, 1::2] = x1[:, : x1[:, 1::2].shape[1] * 2: 2]
        x2 = x1 if M == N else x2
    if kind == "far":  # separations of tens of lengthscales: exp underflows to 0
        x1 = (x1 * 4000.0).astype(np.float32)
        x2 = x1 if M == N else (x2 * 4000.0).astype(np.float32)
    ls = [(0.35 * np.sqrt(D) * 0.5 * (t + 1) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
          for t in range(T)]
    os_ = [(0.6 + 0.6 * g.random(B)).astype(np.float32) for _ in range(T)]
    return x1, x2, ls, os_


def fns_of(names):
    return [covariance.FAMILIES[n] for n in names]


def families_of(names):
    return [covariance.FAMILIES[n].native_family for n in names]


def theta_of(ls, os_, D):
    return K.kernel_sum_theta([dev(a) for a in ls], [dev(a) for a in os_], (ls[0].shape[0],), D)


def dense_sum(names, x1, x2, ls, os_, dtype):
    """sum_t K_t [B, M, N] by the covariance functions in `dtype` on the device (float64: the exact value of the tests;
    float32: the torch composition whose error sets the bound)."""
    a, b = dev(x1, dtype), dev(x2, dtype)
    return sum(fn(a, b, dev(l, dtype), dev(o, dtype)) for fn, l, o in zip(fns_of(names), ls, os_))


def never_called(fn):
    """A covar_func of the same native family that must not be evaluated."""
    def covar(*args, **kwargs):
        raise AssertionError("covar_func was called")

    covar.native_family = fn.native_family
    return covar


def kernel_ops(names, tx1, tx2, tls, tos, spy=True):
    return [KernelLinearOperator(tx1, tx2, never_called(fn) if spy else fn, num_nonbatch_dimensions=NB, lengthscale=l,
                                 outputscale=o) for fn, l, o in zip(fns_of(names), tls, tos)]


def total(ops):
    out = ops[0]
    for op in ops[1:]:
        out = out + op
    return out


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_sum {label}: err {err:.3e} torch fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


# (families, B, M, N, D, c, ARD, diagonal): T = 1 .. 4 with all four families mixed, every D of {1, 3, 8, 32}, every N of
# {1, 63, 257, 1013} (one tile, ragged tile, several tiles, split columns), every c of {1, 4, 17, 33}, B 1 and 3, both
# rectangular orientations, the three diagonal modes
PRODUCT_CASES = [
    (("rbf",), 1, 1, 1, 1, 1, False, "none"),
    (("matern52",), 3, 257, 257, 8, 17, True, "full"),
    (("rbf", "matern52"), 3, 63, 63, 3, 4, True, "full"),
    (("matern12", "matern32"), 1, 257, 257, 1, 33, False, "const"),
    (("matern32", "rbf"), 1, 1013, 1013, 32, 1, True, "none"),
    (("matern52", "matern12"), 1, 1, 1, 8, 4, False, "const"),
    (("matern12", "matern32", "rbf"), 1, 1013, 1013, 8, 17, False, "full"),
    (("rbf", "rbf", "matern52"), 3, 257, 257, 3, 1, True, "none"),
    (("matern52", "matern32", "matern12"), 1, 63, 63, 32, 33, True, "const"),
    (("rbf", "matern12", "matern32", "matern52"), 1, 257, 257, 3, 4, True, "none"),
    (("matern52", "matern32", "matern12", "rbf"), 3, 1013, 1013, 1, 17, False, "const"),
    (("matern32", "matern32", "rbf", "matern12"), 1, 63, 63, 32, 1, True, "full"),
    (("rbf", "matern52", "matern12", "matern32"), 1, 1, 1, 32, 33, False, "none"),
    (("rbf", "matern52"), 3, 130, 77, 3, 4, True, "none"),
    (("matern12", "matern32", "rbf"), 1, 77, 130, 8, 17, False, "none"),
    (("matern52", "rbf", "matern32", "matern12"), 1, 130, 77, 32, 1, True, "none"),
    (("matern32", "matern12"), 3, 77, 130, 1, 33, False, "none"),
]


def product_check(names, x1, x2, ls, os_, v, d, diag, label):
    """lo_kernel_sum_mv_f32 and the sum operator's _matmul against float64; the bound from the torch float32 composition."""
    B, M, D = x1.shape
    N = x2.shape[1]
    want = host(dense_sum(names, x1, x2, ls, os_, torch.float64) @ dev(v, torch.float64))
    comp = dense_sum(names, x1, x2, ls, os_, torch.float32) @ dev(v)
    dd = None
    if diag == "full":
        dd = d
        want = want + d[:, :, None].astype(np.float64) * v
        comp = comp + dev(dd)[:, :, None] * dev(v)
    elif diag == "const":
        dd = d[:, 0]
        want = want + d[:, :1, None].astype(np.float64) * v
        comp = comp + dev(dd)[:, None, None] * dev(v)
    tx1 = dev(x1)
    tx2 = tx1 if x2 is x1 else dev(x2)
    tv = dev(v)
    y = K.kernel_sum_mv(tx1, tx2, theta_of(ls, os_, D), families_of(names), tv, None if dd is None else dev(dd),
                        const_diag=diag == "const")
    assert torch.isfinite(y).all()
    within(f"mv {label}", rel(host(y), want), rel(host(comp), want))
    if len(names) < 2:
        return y
    # the operator: the same kernel through _matmul (rectangular, or square without a diagonal) or through the kind
    ops = kernel_ops(names, tx1, tx2, [dev(a) for a in ls], [dev(a) for a in os_])
    S = total(ops)
    if dd is None:
        assert torch.equal(S._matmul(tv), y)
        desc = S._kernel_descriptor()
        assert (desc is not None) == (x2 is x1)
        if desc is not None:
            assert desc.kind == _hip.LO_OP_KERNEL_SUM_DIAG and desc.kernel_terms == len(names)
    else:
        diag_op = DiagLinearOperator(dev(dd)) if diag == "full" else ConstantDiagLinearOperator(dev(dd)[:, None], N)
        A = AddedDiagLinearOperator(S, diag_op)
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_SUM_DIAG and desc.diag_mode == (1 if diag == "full" else 2)
        assert torch.equal(A._matmul(tv), y)
    return y


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=lambda c: "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in c))
def test_product_against_fp64(case):
    names, B, M, N, D, c, ard, diag = case
    seed = 8000 + 7 * PRODUCT_CASES.index(case)
    x1, x2, ls, os_ = make_points(seed, B, M, N, D, len(names), ard)
    g = rng(seed + 1)
    v = g.standard_normal((B, N, c)).astype(np.float32)
    d = (0.05 + g.random((B, N))).astype(np.float32)
    product_check(names, x1, x2, ls, os_, v, d, diag, "-".join(str(x) for x in case))


@pytest.mark.parametrize("kind", ["dup", "far"])
def test_product_with_coincident_and_with_far_points(kind):
    names = ("rbf", "matern12", "matern32", "matern52")
    B, N, D, c = 1, 257, 3, 4
    x1, x2, ls, os_ = make_points(8300, B, N, N, D, 4, True, kind)
    v = rng(8301).standard_normal((B, N, c)).astype(np.float32)
    y = product_check(names, x1, x2, ls, os_, v, None, "none", f"all-{kind}")
    if kind == "far":  # only the diagonal survives: y = (sum_t os_t^2) v
        os2 = sum(o.astype(np.float64) ** 2 for o in os_)
        assert rel(host(y), os2[:, None, None] * v) <= 1e-6


def test_product_without_a_column_split():
    """B ceil(M / 256) >= 512 workgroups: one workgroup sweeps all the tiles of its rows (no partials, no second pass)."""
    names = ("matern32", "rbf")
    B, M, N, D, c = 128, 1024, 300, 1, 5
    assert _hip.load().lo_kernel_sum_mv_workspace_bytes(B, M, N, D, 2, 17) == 256
    x1, x2, ls, os_ = make_points(8400, B, M, N, D, 2, True)
    v = rng(8401).standard_normal((B, N, c)).astype(np.float32)
    product_check(names, x1, x2, ls, os_, v, None, "none", "no-split")


def test_one_term_agrees_with_the_single_term_kernel():
    B, N, D, c = 3, 1013, 8, 5
    for name in FAMILY_NAMES:
        x1, _, ls, os_ = make_points(8450, B, N, N, D, 1, True)
        v = rng(8451).standard_normal((B, N, c)).astype(np.float32)
        want = host(dense_sum((name,), x1, x1, ls, os_, torch.float64) @ dev(v, torch.float64))
        tx, fam = dev(x1), covariance.FAMILIES[name].native_family
        single = K.kernel_mv(tx, tx, K.kernel_theta(dev(ls[0]), dev(os_[0]), (B,), D), fam, dev(v))
        fused = K.kernel_sum_mv(tx, tx, theta_of(ls, os_, D), [fam], dev(v))
        err, ref_err = rel(host(fused), want), max(rel(host(single), want), ERR_FLOOR)
        print(f"kernel_sum T=1 {name}: err {err:.3e} lo_kernel_mv_f32 {ref_err:.3e} ratio {err / ref_err:.2f}")
        assert err <= REF_FACTOR * ref_err


# (families, B, M, N, D, t, ARD, kind): t of {1, 2, 9} (more than one sweep of 8 columns), duplicated points, points tens of
# lengthscales apart, every padded D, both sweeps of the derivative at 16 < D (T = 3, 4), rectangular pairs
DERIVATIVE_CASES = [
    (("rbf", "matern52"), 1, 257, 257, 3, 1, True, "plain"),
    (("matern12", "matern32", "rbf"), 3, 130, 77, 1, 9, False, "plain"),
    (("matern52", "rbf", "matern12", "matern32"), 1, 77, 130, 8, 2, True, "plain"),
    (("matern32", "matern12", "rbf"), 1, 63, 63, 32, 2, False, "plain"),
    (("rbf", "matern12", "matern32", "matern52"), 1, 40, 300, 20, 1, True, "plain"),
    (("rbf", "matern12", "matern32", "matern52"), 1, 64, 64, 2, 9, True, "dup"),
    (("matern12", "matern52"), 1, 1013, 1013, 13, 2, True, "plain"),
    (("rbf", "matern12", "matern32", "matern52"), 1, 257, 257, 3, 2, True, "far"),
]


def autograd_all(names, x1, x2, ls, os_, U, V, dtype, pm=None, pn=None):
    """Gradients of sum_s u_s^T (sum_t K_t) v_s through the dense covariance functions in `dtype`: (x1, x2 as separate
    leaves, [lengthscale_t], [outputscale_t]).  pm / pn: the order in which the points are taken (the same sums rounded
    along another path); the points' gradients come back in the ORIGINAL order."""
    M, N = x1.shape[1], x2.shape[1]
    pm = np.arange(M) if pm is None else pm
    pn = np.arange(N) if pn is None else pn
    a, b = dev(x1[:, pm], dtype).requires_grad_(True), dev(x2[:, pn], dtype).requires_grad_(True)
    tl = [dev(l, dtype).requires_grad_(True) for l in ls]
    to = [dev(o, dtype).requires_grad_(True) for o in os_]
    Ksum = sum(fn(a, b, l, o) for fn, l, o in zip(fns_of(names), tl, to))
    (dev(U[:, pm], dtype) * (Ksum @ dev(V[:, pn], dtype))).sum().backward()
    ga, gb = np.empty_like(host(a.grad)), np.empty_like(host(b.grad))
    ga[:, pm], gb[:, pn] = host(a.grad), host(b.grad)
    return ga, gb, [host(l.grad) for l in tl], [host(o.grad) for o in to]


@pytest.mark.parametrize("case", DERIVATIVE_CASES, ids=lambda c: "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in c))
def test_derivatives_against_fp64_autograd(case):
    """lo_kernel_sum_bilinear_f32 and lo_kernel_sum_points_grad_f32 behind SumLinearOperator._bilinear_derivative: every
    term's lengthscale and outputscale gradient and the points' gradients of both sides against float64 autograd.  The
    bound of a hyperparameter gradient is the root mean square of float32 autograd's error over REF_ORDERS orderings of
    the points (one number per member: a single draw can land near zero), that of the points' gradients one float32
    evaluation, as in the single-term tests."""
    names, B, M, N, D, t, ard, kind = case
    T = len(names)
    label = "-".join(str(x) for x in case)
    x1, x2, ls, os_ = make_points(8600 + DERIVATIVE_CASES.index(case), B, M, N, D, T, ard, kind)
    same = x2 is x1
    g = rng(8650)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    gx1_64, gx2_64, gl64, go64 = autograd_all(names, x1, x2, ls, os_, U, V, torch.float64)
    ref32 = []
    for k in range(REF_ORDERS):
        pm = rng(8660 + k).permutation(M)
        pn = pm if same else rng(8680 + k).permutation(N)
        ref32.append(autograd_all(names, x1, x2, ls, os_, U, V, torch.float32, pm, pn))
    rms = lambda pick, want: float(np.sqrt(np.mean([rel(pick(r), want) ** 2 for r in ref32])))  # noqa: E731
    # the operator: every tensor asks for a gradient; x1 and x2 one leaf when the points are shared
    lx1 = dev(x1).requires_grad_(True)
    lx2 = lx1 if same else dev(x2).requires_grad_(True)
    tl = [dev(a).requires_grad_(True) for a in ls]
    to = [dev(a).requires_grad_(True) for a in os_]
    S = total(kernel_ops(names, lx1, lx2, tl, to))
    tU, tV = dev(U), dev(V)
    # the route: the fused sweep where it was measured at least as fast, else one single-term call per term
    spies = {n: mock.patch.object(K, n, wraps=getattr(K, n)) for n in
             ("kernel_bilinear", "kernel_points_grad", "kernel_sum_bilinear", "kernel_sum_points_grad")}
    with spies["kernel_bilinear"] as bil, spies["kernel_points_grad"] as pg, spies["kernel_sum_bilinear"] as sbil, \
            spies["kernel_sum_points_grad"] as spg:
        grads = S._bilinear_derivative(tU, tV)
    fused_b, fused_p = K.kernel_sum_fused_bilinear(D, T), K.kernel_sum_fused_points_grad(D, T)
    assert (sbil.call_count, bil.call_count) == ((1, 0) if fused_b else (0, T))
    assert (spg.call_count, pg.call_count) == ((2, 0) if fused_p else (0, 2 * T))
    assert len(grads) == 4 * T
    for k in range(T):
        gx1, gx2, gl, go = grads[4 * k: 4 * k + 4]
        assert (gx1 is not None) == (k == 0) and (gx2 is not None) == (k == 0)  # (the total sits in the first slots)
        assert gl.shape == tl[k].shape and go.shape == to[k].shape
        assert torch.isfinite(gl).all() and torch.isfinite(go).all()
        if kind == "far":  # nothing but the diagonal survives: d / d lengthscale is 0 at the scale of float32
            print(f"kernel_sum bilinear {label} lengthscale{k}: max |g| {np.abs(host(gl)).max():.3e}")
            assert np.abs(host(gl) - gl64[k]).max() <= ERR_FLOOR
        else:
            within(f"bilinear {label} lengthscale{k}", rel(host(gl), gl64[k]), rms(lambda r: r[2][k], gl64[k]))
        within(f"bilinear {label} outputscale{k}", rel(host(go), go64[k]), rms(lambda r: r[3][k], go64[k]))
    gx1, gx2 = grads[0], grads[1]
    assert gx1.shape == lx1.shape and gx2.shape == lx2.shape and torch.isfinite(gx1).all() and torch.isfinite(gx2).all()
    if kind == "far":
        print(f"kernel_sum points {label}: max |g| {np.abs(host(gx1)).max():.3e}")
        assert np.abs(host(gx1) - gx1_64).max() <= ERR_FLOOR and np.abs(host(gx2) - gx2_64).max() <= ERR_FLOOR
    else:
        plain32 = autograd_all(names, x1, x2, ls, os_, U, V, torch.float32)
        within(f"points {label} x1", rel(host(gx1), gx1_64), rel(plain32[0], gx1_64))
        within(f"points {label} x2", rel(host(gx2), gx2_64), rel(plain32[1], gx2_64))
    # the fused entry points themselves, whatever the route of the operator: the same bounds (the same bits where the
    # operator took them)
    theta, fams = theta_of(ls, os_, D), families_of(names)
    tx1 = dev(x1)
    tx2 = tx1 if same else dev(x2)
    f1 = K.kernel_sum_points_grad(tx1, tx2, theta, fams, tU, tV)
    f2 = K.kernel_sum_points_grad(tx2, tx1, theta, fams, tV, tU)
    gt = K.kernel_sum_bilinear(tx1, tx2, theta, fams, tU, tV)
    assert gt.shape == (B, T, D + 1) and torch.isfinite(gt).all()
    if fused_p:
        assert torch.equal(f1, gx1) and torch.equal(f2, gx2)
    if kind == "far":
        assert np.abs(host(f1) - gx1_64).max() <= ERR_FLOOR and np.abs(host(f2) - gx2_64).max() <= ERR_FLOOR
    else:
        within(f"points_grad entry {label} x1", rel(host(f1), gx1_64), rel(plain32[0], gx1_64))
        within(f"points_grad entry {label} x2", rel(host(f2), gx2_64), rel(plain32[1], gx2_64))
    for k in range(T):
        go_k = 2.0 * to[k].detach() * gt[:, k, D]
        if fused_b:
            assert torch.equal(grads[4 * k + 3], go_k)
        within(f"bilinear entry {label} outputscale{k}", rel(host(go_k), go64[k]), rms(lambda r: r[3][k], go64[k]))
        if kind != "far":
            d_ls = (-(theta[:, k, :D] ** 2) * gt[:, k, :D]).reshape(B, 1, D)
            d_ls = d_ls if ard or D == 1 else d_ls.sum(-1, keepdim=True)
            within(f"bilinear entry {label} lengthscale{k}", rel(host(d_ls), gl64[k]), rms(lambda r: r[2][k], gl64[k]))


def test_only_the_tensors_that_ask_get_a_gradient():
    names = ("rbf", "matern32")
    B, N, D, t = 1, 130, 3, 2
    x1, _, ls, os_ = make_points(8700, B, N, N, D, 2, True)
    tx = dev(x1)
    tl = [dev(ls[0]), dev(ls[1]).requires_grad_(True)]
    to = [dev(a) for a in os_]
    S = total(kernel_ops(names, tx, tx, tl, to))
    U, V = torch.randn(B, N, t, device=DEV), torch.randn(B, N, t, device=DEV)
    with mock.patch.object(K, "kernel_sum_points_grad", side_effect=AssertionError("points' gradient")), \
            mock.patch.object(K, "kernel_points_grad", side_effect=AssertionError("points' gradient")):
        grads = S._bilinear_derivative(U, V)
    assert [g is not None for g in grads] == [False, False, False, False, False, False, True, False]
    none = total(kernel_ops(names, tx, tx, [dev(a) for a in ls], to))
    with mock.patch.object(K, "kernel_sum_bilinear", side_effect=AssertionError("derivative")), \
            mock.patch.object(K, "kernel_bilinear", side_effect=AssertionError("derivative")):
        assert all(g is None for g in none._bilinear_derivative(U, V))


@pytest.mark.parametrize("shape", [(3, 1013, 700, 8, 5), (512, 40, 40, 2, 2)], ids=["split", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, M, N, D, t = shape
    names = ("rbf", "matern12", "matern52")
    x1, x2, ls, os_ = make_points(8500, B, M, N, D, 3, True)
    tx1, tx2, theta, fams = dev(x1), dev(x2), theta_of(ls, os_, D), families_of(names)
    assert (_hip.load().lo_kernel_sum_mv_workspace_bytes(B, M, N, D, 3, 17) > 256) == (M == 1013)
    U, V = torch.randn(B, M, t, device=DEV), torch.randn(B, N, t, device=DEV)
    for fn, args in ((K.kernel_sum_mv, (V,)), (K.kernel_sum_bilinear, (U, V)), (K.kernel_sum_points_grad, (U, V))):
        assert torch.equal(fn(tx1, tx2, theta, fams, *args), fn(tx1, tx2, theta, fams, *args)), fn.__name__


def test_error_codes_of_the_entry_points():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, c, T = 1, 300, 300, 3, 2, 2
    x = torch.rand(B, M, D, device=DEV)
    theta = torch.ones(B, T, D + 1, device=DEV)
    v, U = torch.randn(B, N, c, device=DEV), torch.randn(B, M, c, device=DEV)
    y = torch.full((B, M, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    fam = (ctypes.c_int32 * 4)(0, 3, 1, 2)
    need = lib.lo_kernel_sum_mv_workspace_bytes(B, M, N, D, T, c)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(x1=x, xb=x, th=theta, fm=fam, tt=T, b=B, m=M, n=N, dim=D, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_sum_mv_f32(p(x1), p(xb), p(th), fm, tt, b, m, n, dim, p(vv), cc, p(dd), mode, p(yy), p(w),
                                        wb, st)

    assert mv() == 0
    torch.cuda.synchronize()
    y.fill_(-7.0)
    bad_fam, neg_fam = (ctypes.c_int32 * 2)(0, 4), (ctypes.c_int32 * 2)(-1, 0)
    for bad in (dict(x1=None), dict(xb=None), dict(th=None), dict(fm=None), dict(vv=None), dict(yy=None), dict(b=0),
                dict(m=0), dict(n=-1), dict(dim=0), dict(cc=0), dict(tt=0), dict(tt=5), dict(fm=bad_fam),
                dict(fm=neg_fam), dict(mode=1), dict(mode=2), dict(mode=3)):
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    wide, th33 = torch.rand(1, 10, 33, device=DEV), torch.ones(1, T, 34, device=DEV)
    v10, y10 = torch.randn(1, 10, 1, device=DEV), torch.full((1, 10, 1), -7.0, device=DEV)
    assert mv(x1=wide, xb=wide, th=th33, m=10, n=10, dim=33, vv=v10, cc=1, yy=y10) == _hip.LO_ERR_UNSUPPORTED
    # a short workspace is refused before anything is launched: y keeps its fill (as after every refusal above)
    assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((y10 == -7.0).all())
    # the derivative and the points' gradient
    for name, out in (("bilinear", torch.full((B, T, D + 1), -7.0, device=DEV)),
                      ("points_grad", torch.full((B, M, D), -7.0, device=DEV))):
        sizer, entry = getattr(lib, f"lo_kernel_sum_{name}_workspace_bytes"), getattr(lib, f"lo_kernel_sum_{name}_f32")
        gneed = sizer(B, M, N, D, T, c)
        gws = torch.empty(gneed, dtype=torch.uint8, device=DEV)

        def call(x1=x, th=theta, fm=fam, tt=T, dim=D, uu=U, vv=v, t=c, gg=out, w=gws, wb=gneed):
            return entry(p(x1), p(x), p(th), fm, tt, B, M, N, dim, p(uu), p(vv), t, p(gg), p(w), wb, st)

        assert call() == 0
        torch.cuda.synchronize()
        out.fill_(-7.0)
        for bad in (dict(x1=None), dict(th=None), dict(fm=None), dict(uu=None), dict(vv=None), dict(gg=None), dict(t=0),
                    dict(tt=0), dict(tt=5), dict(fm=bad_fam), dict(dim=0)):
            assert call(**bad) == -1, (name, bad)
        assert call(dim=33) == _hip.LO_ERR_UNSUPPORTED and sizer(B, M, N, 33, T, c) == 0
        assert call(wb=gneed - 1) == -3 and call(w=None, wb=0) == -3
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), name


def test_error_codes_of_the_kind():
    """LO_OP_KERNEL_SUM_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; the float64
    entry points refuse the kind, and a sum that holds a kernel term."""
    lib, p = _hip.load(), _hip.ptr
    B, N, D, c = 1, 300, 3, 2
    x = torch.rand(B, N, D, device=DEV)
    theta = torch.ones(B, 2, D + 1, device=DEV)
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_sum_diag_descriptor(x, theta, [0, 3])
    assert desc.kind == _hip.LO_OP_KERNEL_SUM_DIAG and desc.n2 == 0x30 and desc.R == D
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_sum_mv(x, x, theta, [0, 3], v))
    y.fill_(-7.0)
    for field, val, rc in (("n2", 0x40, -1), ("n2", 0x130, -1), ("n2", -1, -1), ("nterms", 0, -1), ("nterms", 5, -1),
                           ("A1", None, -1), ("R", 0, -1), ("R", 33, _hip.LO_ERR_UNSUPPORTED)):
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_sum_diag_descriptor(torch.rand(1, 10, 33, device=DEV), torch.ones(1, 2, 34, device=DEV), [0, 1]) is None
    # the pivoted Cholesky
    L, perm = torch.empty(B, 5, N, device=DEV), torch.empty(B, N, dtype=torch.int64, device=DEV)
    rank = ctypes.c_int32(0)
    root = K.lowrank_diag_descriptor(torch.rand(B, N, 4, device=DEV), None)
    both = K.sum_descriptor([desc, root]).c_struct()
    pneed = max(lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(s), 5),
                lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(both), 5))
    pws = torch.empty(pneed, dtype=torch.uint8, device=DEV)
    args = (5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed, st)
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == 0 and rank.value == 5
    for field, val, rc in (("n2", 0x40, -1), ("nterms", 5, -1), ("R", 33, _hip.LO_ERR_UNSUPPORTED)):
        s = desc.c_struct()
        setattr(s, field, val)
        assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed,
                                       st) == _hip.LO_ERR_UNSUPPORTED
    y64 = torch.empty(B, N, c, dtype=torch.float64, device=DEV)
    assert lib.lo_matvec_f64(ctypes.byref(s), p(v.double()), p(y64), c, p(ws), need, st) == _hip.LO_ERR_UNSUPPORTED
    # a sum with a kernel term: taken by the float32 entry points, refused by the float64 ones
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(both), *args) == 0
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(both), 5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed,
                                       st) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_matvec_f64(ctypes.byref(both), p(v.double()), p(y64), c, p(ws), need, st) == _hip.LO_ERR_UNSUPPORTED
    assert K.masked_descriptor(K.sum_descriptor([desc, root]), torch.arange(0, N, 2, device=DEV)) is None


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g39_kernel_sum_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in t:
            if k == "x" or k.startswith(("lengthscale", "outputscale")):
                t[k].requires_grad_(True)
    return t


def kernel_sum(p, t):
    """K_1 + .. + K_T of case p over the ONE tensor t["x"], every covar_func a spy that raises."""
    names = CASES[p][0]
    return total(kernel_ops(names, t["x"], t["x"], [t[f"lengthscale{k}"] for k in range(len(names))],
                            [t[f"outputscale{k}"] for k in range(len(names))]))


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_sum {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(kernel_sum(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(K_1 + .. + K_T + Diag) under the reference run's solver settings, every covar_func a spy: the descriptor kind, the
    product, solve, inv_quad_logdet with injected probes, the pivoted Cholesky and backward."""
    G = golden(p)
    T = len(CASES[p][0])
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = kernel_sum(p, t)
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_SUM_DIAG and desc.kernel_terms == T and desc.diag_mode == 1
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.A1.shape == (CASES[p][1], T, CASES[p][3] + 1)
        assert (S + DiagLinearOperator(t["noise"]))._kernel_descriptor().kind == _hip.LO_OP_KERNEL_SUM_DIAG
        check(G, p, "mv", S @ t["V"])
        check(G, p, "solve", A.solve(t["rhs"]))
        iq, ld = probed(p, t).inv_quad_logdet(t["rhs"], logdet=True)
        check(G, p, "iq", iq)
        check(G, p, "ld", ld)
        L, piv = S.pivoted_cholesky(RANK, return_pivots=True)
        L2, piv2 = S.pivoted_cholesky(RANK, return_pivots=True)
        assert np.array_equal(piv[..., :RANK].cpu().numpy(), G["piv"])
        check(G, p, "L", L)
        assert torch.equal(L, L2) and torch.equal(piv, piv2)
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(kernel_sum(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    for k in range(T):
        check(G, p, f"gl{k}", tg[f"lengthscale{k}"].grad)
        check(G, p, f"go{k}", tg[f"outputscale{k}"].grad)
    check(G, p, "gx", tg["x"].grad)


def test_kernel_plus_low_rank_root_plus_diagonal_lowers_to_a_sum_with_a_kernel_term():
    """RBF + a linear kernel (a low-rank root) + noise: LO_OP_SUM with a kernel term; its solve against a dense float64
    solve, within 4 times the error of the parent's route -- the same operator with the descriptor patched to None (a
    Python call per product, one kernel product and one root product per call)."""
    B, N, D, R = 1, 700, 3, 5
    x1, _, ls, os_ = make_points(8800, B, N, N, D, 1, True)
    g = rng(8801)
    C = (0.3 * g.standard_normal((B, N, R))).astype(np.float32)
    noise = (0.05 + 0.1 * g.random((B, N))).astype(np.float32)
    rhs = g.standard_normal((B, N, 2)).astype(np.float32)
    A64 = dense_sum(("rbf",), x1, x1, ls, os_, torch.float64) + dev(C, torch.float64) @ dev(C, torch.float64).mT \
        + torch.diag_embed(dev(noise, torch.float64))
    want = host(torch.linalg.solve(A64, dev(rhs, torch.float64)))

    def build(spy=True):
        tx = dev(x1)
        kern = kernel_ops(("rbf",), tx, tx, [dev(ls[0])], [dev(os_[0])], spy)[0]
        return AddedDiagLinearOperator(kern + LowRankRootLinearOperator(dev(C)), DiagLinearOperator(dev(noise)))

    with solver_settings(settings):
        A = build()
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_SUM and desc.diag_mode == 1
        assert [t.kind for t in desc.terms] == [_hip.LO_OP_KERNEL_DIAG, _hip.LO_OP_LOWRANK_DIAG]
        got = A.solve(dev(rhs))
        with mock.patch.object(AddedDiagLinearOperator, "_kernel_descriptor", return_value=None), \
                mock.patch.object(SumLinearOperator, "_kernel_descriptor", return_value=None):
            parent = build(spy=False).solve(dev(rhs))  # (the generic pivoted Cholesky fetches rows through covar_func)
    within("kernel + root + diag solve", rel(host(got), want), rel(host(parent), want))
    # two kernel operators over DIFFERENT point tensors of one shape: two kernel terms of LO_OP_SUM
    ta, tb = dev(x1), dev(x1[:, ::-1].copy())
    two = kernel_ops(("rbf", "matern32"), ta, ta, [dev(ls[0])] * 2, [dev(os_[0])] * 2)
    two[1] = kernel_ops(("matern32",), tb, tb, [dev(ls[0])], [dev(os_[0])])[0]
    S = two[0] + two[1]
    desc = S._kernel_descriptor()
    assert desc.kind == _hip.LO_OP_SUM and [t.kind for t in desc.terms] == [_hip.LO_OP_KERNEL_DIAG] * 2
    v = dev(rhs)
    assert torch.allclose(S._matmul(v), two[0]._matmul(v) + two[1]._matmul(v), rtol=1e-5, atol=1e-5)


def test_rectangular_sum_product_is_one_fused_call():
    """The prediction product K(x*, X) alpha of a sum: one lo_kernel_sum_mv_f32 call, no per-term call, equal to
    sum(op._matmul(v)) within the bound; the transposed product likewise."""
    names = ("rbf", "matern52", "matern12")
    B, M, N, D, c = 3, 130, 77, 3, 4
    x1, x2, ls, os_ = make_points(8900, B, M, N, D, 3, True)
    v = rng(8901).standard_normal((B, N, c)).astype(np.float32)
    w = rng(8902).standard_normal((B, M, c)).astype(np.float32)
    Kd = dense_sum(names, x1, x2, ls, os_, torch.float64)
    ops = kernel_ops(names, dev(x1), dev(x2), [dev(a) for a in ls], [dev(a) for a in os_])
    S = total(ops)
    assert S._kernel_descriptor() is None
    per_term = sum(op._matmul(dev(v)) for op in ops)
    per_term_t = sum(op._t_matmul(dev(w)) for op in ops)
    with mock.patch.object(K, "kernel_mv", side_effect=AssertionError("per-term product")), \
            mock.patch.object(K, "kernel_sum_mv", wraps=K.kernel_sum_mv) as spy:
        y, yt = S._matmul(dev(v)), S._t_matmul(dev(w))
    assert spy.call_count == 2 and y.shape == (B, M, c) and yt.shape == (B, N, c)
    want, want_t = host(Kd @ dev(v, torch.float64)), host(Kd.mT @ dev(w, torch.float64))
    within("rectangular sum product", rel(host(y), want), rel(host(per_term), want))
    within("rectangular sum product, transposed", rel(host(yt), want_t), rel(host(per_term_t), want_t))
