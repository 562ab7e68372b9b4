"""The matrix-free task-indexed ("Hadamard") multitask operator on the MI355X: lo_kernel_task_mv_f32 /
lo_kernel_task_bilinear_f32 / lo_kernel_task_points_grad_f32 (csrc/lo_kernel_task.hip) against the float64 dense
composition, the kind LO_OP_KERNEL_TASK_DIAG through the public API (product, diagonal, solve, inv_quad_logdet, pivoted
Cholesky, gradients) against the reference's goldens (tests/golden/g43_kernel_task_*.npz), its error codes and refusals,
and its memory.

Bounds: the protocol of tests/test_gpu_kernel_op.py and test_gpu_kernel_kron.py.  Direct entry points: the error against
the float64 dense composition (for the derivatives: float64 autograd through it) is at most REF_FACTOR = 4 times the error
of the torch float32 dense composition on the same inputs, floored at ERR_FLOOR = 1e-7.  Golden quantities: 4 times the
reference's own recorded float32 error.  Gradients through inv_quad: 4 times the error of the float32 run of the same
computation on the STORED dense operator.  Every test prints the ratio it measured (DESIGN.md section 6q holds the
table).  No test feeds a task id outside [0, T)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_task import (  # noqa: E402
    CASES, ERR_FLOOR, GRAD_NAMES, PROBES, RANK, inputs, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_task {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def task_fn(name):
    return covariance.TASK_FAMILIES[name + "_task"]


def guarded(fn, n):
    """A covar_func of the same native family and outputs that fails on any dense evaluation: both arguments with all n
    points."""
    def covar(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError(f"covar_func was evaluated densely: {tuple(x1.shape)} x {tuple(x2.shape)}")
        return fn(x1, x2, **params)

    covar.native_family, covar.native_outputs = fn.native_family, fn.native_outputs
    return covar


def make_points(g, B, n, D, T, kind="plain", absent=None):
    """[B, n, D + 1]: D coordinates and the task id; ids uneven (task t drawn with weight t + 1), `absent` never drawn."""
    x = g.random((B, n, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with r = 0 off the diagonal
        x[:, 1::2] = x[:, : x[:, 1::2].shape[1] * 2: 2]
    if kind == "far":  # separations of thousands of lengthscales: every off-diagonal kernel value underflows to 0
        x = (x * 4000.0).astype(np.float32)
        x[:, :, 0] += 4000.0 * np.arange(n, dtype=np.float32)[None, :]
    w = np.arange(1, T + 1, dtype=np.float64)
    if absent is not None:
        w[absent] = 0.0
    ids = g.choice(T, size=(B, n), p=w / w.sum())
    return np.concatenate([x, ids[..., None].astype(np.float32)], -1)


def make_inputs(seed, B, M, N, D, T, c, ard=True, kind="plain", absent=None):
    """Points of both sides (one array when M == N), hyperparameters, a NON-symmetric Bt, columns and a full diagonal."""
    g = rng(seed)
    x1 = make_points(g, B, M, D, T, kind, absent)
    x2 = x1 if M == N else make_points(g, B, N, D, T, kind, absent)
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    Bt = (np.eye(T) * (1.0 + 0.3 * np.arange(T)) + 0.5 * (g.random((B, T, T)) - 0.3) * (1 - np.eye(T))).astype(np.float32)
    v = g.standard_normal((B, N, c)).astype(np.float32)
    d = (0.05 + g.random((B, N))).astype(np.float32)
    return x1, x2, ls, os_, Bt, v, d


def composition(fn, x1, x2, ls, os_, Bt, v, d, diag, dtype):
    """K(x1, x2) v + d o v with K stored densely, in `dtype` on the device."""
    A = fn(dev(x1, dtype), dev(x2, dtype), dev(ls, dtype), dev(os_, dtype), dev(Bt, dtype))
    y = A @ dev(v, dtype)
    if diag == "full":
        y = y + dev(d, dtype)[:, :, None] * dev(v, dtype)
    elif diag == "const":
        y = y + dev(d[:, :1], dtype)[:, :, None] * dev(v, dtype)
    return y


def theta_of(ls, os_, D):
    return K.kernel_theta(dev(ls), dev(os_), (ls.shape[0],), D)


def direct(fn, x1, x2, ls, os_, Bt, v, d, diag):
    D = x1.shape[-1] - 1
    dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
    tx1 = dev(x1)
    tx2 = tx1 if x2 is x1 else dev(x2)
    return K.kernel_task_mv(tx1, tx2, theta_of(ls, os_, D), dev(Bt), fn.native_family, dev(v), dd,
                            const_diag=diag == "const")


def split_expected(B, M, N):
    return not (B * -(-M // 256) >= 512 or N <= 128)


# (family, B, M, N, D, T, c, diagonal, absent task): every family, D of {1, 3, 8, 31} (every padded width), T of
# {1, 2, 3, 8}, c of {1, 4, 17} (every column chunk, a second sweep), n of {1, 63, 130, 257, 300} (one tile, a ragged
# tile, several tiles, two row blocks), B of {1, 3, 512} (split and unsplit columns), rectangular M != N, every diagonal
# mode, a task id without a point
DIRECT_CASES = [
    ("rbf", 3, 257, 257, 3, 2, 1, "full", None),
    ("matern12", 1, 63, 63, 1, 1, 4, "const", None),
    ("matern32", 1, 130, 130, 31, 8, 4, "full", None),
    ("matern52", 1, 300, 300, 8, 3, 17, "none", None),
    ("matern52", 1, 300, 300, 8, 3, 17, "full", 1),
    ("rbf", 512, 40, 40, 2, 2, 4, "const", None),
    ("rbf", 1, 1, 1, 1, 1, 1, "none", None),
    ("matern32", 3, 257, 130, 3, 3, 1, "none", None),
    ("matern12", 1, 63, 300, 8, 8, 17, "none", 5),
    ("rbf", 3, 257, 257, 3, 2, 1, "const", None),
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_product_against_the_fp64_composition(case):
    name, B, M, N, D, T, c, diag, absent = case
    fn = task_fn(name)
    x1, x2, ls, os_, Bt, v, d = make_inputs(9600 + DIRECT_CASES.index(case), B, M, N, D, T, c, absent=absent)
    if T > 1:
        assert not np.allclose(Bt, Bt.transpose(0, 2, 1))  # (a transposed lookup would not pass)
    if absent is not None:
        assert not (x1[..., D] == absent).any() and not (x2[..., D] == absent).any()
    lib = _hip.load()
    assert (lib.lo_kernel_task_mv_workspace_bytes(B, M, N, D, T, c) > 256) == split_expected(B, M, N)
    want = host(composition(fn, x1, x2, ls, os_, Bt, v, d, diag, torch.float64))
    comp = host(composition(fn, x1, x2, ls, os_, Bt, v, d, diag, torch.float32))
    y = direct(fn, x1, x2, ls, os_, Bt, v, d, diag)
    assert y.shape == (B, M, c) and torch.isfinite(y).all()
    within("mv " + "-".join(str(a) for a in case), rel(host(y), want), rel(comp, want))
    if M == N:  # the kind through lo_matvec_f32 runs the same kernel: the same bits
        dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
        desc = K.kernel_task_diag_descriptor(dev(x1), theta_of(ls, os_, D), fn.native_family, dev(Bt), dd,
                                             const_diag=diag == "const")
        assert desc.kind == _hip.LO_OP_KERNEL_TASK_DIAG and desc.N == N and desc.R == D and desc.kernel_terms == T
        assert torch.equal(K.matvec(desc, dev(v)), y)


@pytest.mark.parametrize("case", [("rbf", 2, 130, 3, 3, 4), ("matern52", 1, 70, 8, 8, 1)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_product_agrees_with_the_kronecker_kind_on_repeated_points(case):
    """X repeated for every task with ids 0 .. T - 1, index i T + t, is Kernel(X, X) (x) Bt: lo_kernel_kron_mv_f32 on
    (X, Bt) computes the same product.  Both within the bound of the float32 composition."""
    name, B, n, D, T, c = case
    fn = task_fn(name)
    x1, _, ls, os_, Bt, _, _ = make_inputs(9700, B, n, n, D, T, c)
    g = rng(9701)
    X = x1[..., :D]
    rep = np.concatenate([np.repeat(X, T, axis=1), np.tile(np.arange(T, dtype=np.float32), n)[None, :, None].repeat(B, 0)], -1)
    v = g.standard_normal((B, n * T, c)).astype(np.float32)
    want = host(composition(fn, rep, rep, ls, os_, Bt, v, None, "none", torch.float64))
    comp = host(composition(fn, rep, rep, ls, os_, Bt, v, None, "none", torch.float32))
    y = direct(fn, rep, rep, ls, os_, Bt, v, None, "none")
    ykron = K.kernel_kron_mv(dev(X), theta_of(ls, os_, D), dev(Bt), fn.native_family, dev(v))
    within("mv repeated points " + name, rel(host(y), want), rel(comp, want))
    within("kron on the same " + name, rel(host(ykron), want), rel(comp, want))
    within("task against kron " + name, rel(host(y), host(ykron)), rel(comp, want))


@pytest.mark.parametrize("kind", ["dup", "far"])
def test_product_with_coincident_and_with_far_points(kind):
    name, B, n, D, T, c = "matern52", 1, 130, 3, 3, 4
    fn = task_fn(name)
    x1, x2, ls, os_, Bt, v, d = make_inputs(9800, B, n, n, D, T, c, kind=kind)
    want = host(composition(fn, x1, x2, ls, os_, Bt, v, d, "full", torch.float64))
    comp = host(composition(fn, x1, x2, ls, os_, Bt, v, d, "full", torch.float32))
    y = direct(fn, x1, x2, ls, os_, Bt, v, d, "full")
    assert torch.isfinite(y).all()
    within(f"mv {kind}", rel(host(y), want), rel(comp, want))
    if kind == "far":  # only the diagonal survives: y[i] = (os^2 Bt[t_i, t_i] + d_i) v[i]
        ids = x1[..., D].astype(np.int64)
        own = np.take_along_axis(np.diagonal(Bt, axis1=1, axis2=2).astype(np.float64), ids, 1)
        scale = os_.astype(np.float64)[:, None] ** 2 * own + d
        assert rel(host(y), scale[:, :, None] * v) <= 1e-6


# ---------------------------------------------------------------------------------- the derivatives
def autograd_all(fn, x1, x2, ls, os_, Bt, U, V, dtype):
    """d / d (theta, Bt, x1, x2) of sum_s u_s^T K(x1, x2) v_s by torch autograd in `dtype` through the dense function, with
    theta = (1 / lengthscale, outputscale^2) as the leaf the entry point differentiates by."""
    D = x1.shape[-1] - 1
    B = x1.shape[0]
    inv = (1.0 / dev(ls, dtype)).expand(B, 1, D)[:, 0]
    theta = torch.cat((inv, dev(os_, dtype).square()[:, None]), -1).requires_grad_(True)
    a, b = dev(x1, dtype).requires_grad_(True), dev(x2, dtype).requires_grad_(True)
    tb = dev(Bt, dtype).requires_grad_(True)
    dense = fn(a, b, (1.0 / theta[:, :D])[:, None, :], theta[:, D].sqrt(), tb)
    (dev(U, dtype) * (dense @ dev(V, dtype))).sum().backward()
    return [host(t.grad) for t in (theta, tb, a, b)]


# (family, B, M, N, D, T, t, kind, absent task): the spread of the product's shapes with t of {1, 8, 11} (one sweep of
# the 8 columns, exactly one, a second ragged one)
DERIV_CASES = [
    ("rbf", 3, 257, 257, 3, 2, 1, "plain", None),
    ("matern12", 1, 63, 130, 1, 1, 8, "plain", None),
    ("matern32", 1, 130, 63, 31, 8, 11, "plain", 6),
    ("matern52", 1, 300, 300, 8, 3, 11, "plain", 1),
    ("rbf", 512, 40, 40, 2, 2, 8, "plain", None),
    ("rbf", 1, 1, 1, 1, 1, 1, "plain", None),
    ("matern52", 1, 130, 130, 3, 3, 8, "dup", None),
    ("matern12", 1, 130, 130, 3, 3, 1, "dup", None),
    ("matern32", 1, 130, 130, 3, 3, 8, "far", None),
]


@pytest.mark.parametrize("case", DERIV_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_bilinear_and_points_gradient_against_fp64_autograd(case):
    name, B, M, N, D, T, t, kind, absent = case
    label = "-".join(str(a) for a in case)
    fn = task_fn(name)
    x1, x2, ls, os_, Bt, _, _ = make_inputs(9900 + DERIV_CASES.index(case), B, M, N, D, T, 1, kind=kind, absent=absent)
    g = rng(9950)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    if M == N:  # (x1 is x2 as arrays; as autograd leaves the two sides are apart, as the entry points hold them)
        x2 = x1.copy()
    want = autograd_all(fn, x1, x2, ls, os_, Bt, U, V, torch.float64)
    ref = autograd_all(fn, x1, x2, ls, os_, Bt, U, V, torch.float32)
    tx1, tx2, tB, tU, tV = dev(x1), dev(x2), dev(Bt), dev(U), dev(V)
    theta = theta_of(ls, os_, D)
    fam = fn.native_family
    g_theta, g_task = K.kernel_task_bilinear(tx1, tx2, theta, tB, fam, tU, tV)
    g_x1 = K.kernel_task_points_grad(tx1, tx2, theta, tB, fam, tU, tV)
    g_x2 = K.kernel_task_points_grad(tx2, tx1, theta, tB.mT.contiguous(), fam, tV, tU)
    assert g_theta.shape == (B, D + 1) and g_task.shape == (B, T, T)
    assert g_x1.shape == (B, M, D + 1) and g_x2.shape == (B, N, D + 1)
    for got in (g_theta, g_task, g_x1, g_x2):
        assert torch.isfinite(got).all()
    assert not g_x1[..., D].any() and not g_x2[..., D].any()  # (the task column: exactly 0)
    assert not want[2][..., D].any() and not want[3][..., D].any()
    if absent is not None:  # a task without a point: exact zeros in its row and column
        assert not g_task[:, absent, :].any() and not g_task[:, :, absent].any()
    for what, got, w, r in (("theta", g_theta, want[0], ref[0]), ("task", g_task, want[1], ref[1]),
                            ("x1", g_x1, want[2], ref[2]), ("x2", g_x2, want[3], ref[3])):
        if what in ("x1", "x2") and not np.linalg.norm(w):
            # (every pair coincides or underflows -- one point, far points: the points' gradient is exactly 0)
            assert kind == "far" or M == N == 1
            assert not got.any(), what
            continue
        within(f"{what} {label}", rel(host(got), w), rel(r, w))
    # two calls give the same bits
    again = K.kernel_task_bilinear(tx1, tx2, theta, tB, fam, tU, tV)
    assert torch.equal(again[0], g_theta) and torch.equal(again[1], g_task)
    assert torch.equal(K.kernel_task_points_grad(tx1, tx2, theta, tB, fam, tU, tV), g_x1)


@pytest.mark.parametrize("shape", [(1, 300, 8, 3, 17), (512, 40, 2, 2, 4)], ids=["split", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, n, D, T, c = shape
    fn = task_fn("matern32")
    x1, x2, ls, os_, Bt, v, d = make_inputs(9960, B, n, n, D, T, c)
    lib = _hip.load()
    assert (lib.lo_kernel_task_mv_workspace_bytes(B, n, n, D, T, c) > 256) == (B == 1)
    assert (lib.lo_kernel_task_points_grad_workspace_bytes(B, n, n, D, T, c) > 256) == (B == 1)
    assert torch.equal(direct(fn, x1, x2, ls, os_, Bt, v, d, "full"), direct(fn, x1, x2, ls, os_, Bt, v, d, "full"))
    tx, tB, tV = dev(x1), dev(Bt), dev(v)
    tU = dev(rng(9961).standard_normal((B, n, c)).astype(np.float32))
    theta = theta_of(ls, os_, D)
    a, b = (K.kernel_task_bilinear(tx, tx, theta, tB, fn.native_family, tU, tV) for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p, q = (K.kernel_task_points_grad(tx, tx, theta, tB, fn.native_family, tU, tV) for _ in range(2))
    assert torch.equal(p, q)


# ---------------------------------------------------------------------------------- error codes
def test_error_codes_of_the_entry_points():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, T, c = 1, 300, 3, 2, 2
    x = torch.cat((torch.rand(B, n, D, device=DEV), torch.randint(0, T, (B, n, 1), device=DEV).float()), -1)
    theta = torch.ones(B, D + 1, device=DEV)
    Bt = torch.eye(T, device=DEV).expand(B, T, T).contiguous()
    v = torch.randn(B, n, c, device=DEV)
    y = torch.full((B, n, c), -7.0, device=DEV)
    gt, gB = torch.full((B, D + 1), -7.0, device=DEV), torch.full((B, T, T), -7.0, device=DEV)
    gx = torch.full((B, n, D + 1), -7.0, device=DEV)
    dfull = torch.ones(B, n, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = max(lib.lo_kernel_task_mv_workspace_bytes(B, n, n, D, T, c),
               lib.lo_kernel_task_bilinear_workspace_bytes(B, n, n, D, T, c),
               lib.lo_kernel_task_points_grad_workspace_bytes(B, n, n, D, T, c))
    assert lib.lo_kernel_task_mv_workspace_bytes(B, n, n, D, T, c) > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(xx=x, th=theta, tk=Bt, fam=0, b=B, m=n, nn=n, dim=D, tt=T, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_task_mv_f32(p(xx), p(xx), p(th), p(tk), fam, b, m, nn, dim, tt, p(vv), cc, p(dd), mode, p(yy),
                                         p(w), wb, st)

    def bil(xx=x, th=theta, tk=Bt, fam=0, b=B, m=n, nn=n, dim=D, tt=T, uu=v, vv=v, cc=c, g1=gt, g2=gB, w=ws, wb=need):
        return lib.lo_kernel_task_bilinear_f32(p(xx), p(xx), p(th), p(tk), fam, b, m, nn, dim, tt, p(uu), p(vv), cc, p(g1),
                                               p(g2), p(w), wb, st)

    def pg(xx=x, th=theta, tk=Bt, fam=0, b=B, m=n, nn=n, dim=D, tt=T, uu=v, vv=v, cc=c, g1=gx, w=ws, wb=need):
        return lib.lo_kernel_task_points_grad_f32(p(xx), p(xx), p(th), p(tk), fam, b, m, nn, dim, tt, p(uu), p(vv), cc,
                                                  p(g1), p(w), wb, st)

    assert mv() == 0 and mv(dd=dfull, mode=1) == 0 and bil() == 0 and pg() == 0
    assert mv(m=130, dd=None, mode=1, yy=torch.empty(B, 130, c, device=DEV)) == 0  # (M != N: the diagonal is not read)
    torch.cuda.synchronize()
    for t in (y, gt, gB, gx):
        t.fill_(-7.0)
    shared = (dict(xx=None), dict(th=None), dict(tk=None), dict(vv=None), dict(b=0), dict(m=0), dict(nn=0), dict(nn=-1),
              dict(dim=0), dict(cc=0), dict(tt=0), dict(tt=-1), dict(fam=4), dict(fam=-1))
    for bad in shared + (dict(yy=None), dict(mode=1), dict(mode=2), dict(mode=3)):
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    for bad in shared + (dict(uu=None), dict(g1=None), dict(g2=None)):
        assert bil(**bad) == -1, bad
    for bad in shared + (dict(uu=None), dict(g1=None)):
        assert pg(**bad) == -1, bad
    wide, th33 = torch.zeros(1, 10, 33, device=DEV), torch.ones(1, 33, device=DEV)
    B9 = torch.eye(9, device=DEV).expand(1, 9, 9).contiguous()
    v10 = torch.randn(1, 10, 1, device=DEV)
    y10, gx33 = torch.full((1, 10, 1), -7.0, device=DEV), torch.full((1, 10, 33), -7.0, device=DEV)
    gt33, gB9 = torch.full((1, 33), -7.0, device=DEV), torch.full((1, 9, 9), -7.0, device=DEV)
    for fn_, extra in ((mv, dict(yy=y10)), (bil, dict(uu=v10, g1=gt33)), (pg, dict(uu=v10, g1=gx33))):
        assert fn_(xx=wide, th=th33, m=10, nn=10, dim=32, vv=v10, cc=1, **extra) == _hip.LO_ERR_UNSUPPORTED  # (D + 1 = 33)
    for fn_, extra in ((mv, dict(yy=y10)), (bil, dict(uu=v10, g2=gB9)), (pg, dict(uu=v10))):
        assert fn_(tk=B9, m=10, nn=10, tt=9, vv=v10, cc=1, **extra) == _hip.LO_ERR_UNSUPPORTED
    for sizer in (lib.lo_kernel_task_mv_workspace_bytes, lib.lo_kernel_task_bilinear_workspace_bytes,
                  lib.lo_kernel_task_points_grad_workspace_bytes):
        assert sizer(1, 10, 10, 32, 2, 1) == 0 and sizer(1, 10, 10, 3, 9, 1) == 0
    # a short workspace is refused before anything is launched: the outputs keep their fill (as after every refusal above)
    assert mv(wb=lib.lo_kernel_task_mv_workspace_bytes(B, n, n, D, T, c) - 1) == -3 and mv(w=None, wb=0) == -3
    assert bil(wb=255) == -3 and bil(w=None, wb=0) == -3 and pg(wb=255) == -3 and pg(w=None, wb=0) == -3
    torch.cuda.synchronize()
    for t in (y, gt, gB, gx, y10, gx33, gt33, gB9):
        assert bool((t == -7.0).all())


def test_error_codes_and_refusals_of_the_kind():
    """LO_OP_KERNEL_TASK_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; the float64
    entry points refuse the kind, a sum does not take it as a term and a mask not as its base."""
    lib, p = _hip.load(), _hip.ptr
    B, N, D, T, c = 1, 300, 3, 2, 2
    x = torch.cat((torch.rand(B, N, D, device=DEV), torch.randint(0, T, (B, N, 1), device=DEV).float()), -1)
    theta = torch.ones(B, D + 1, device=DEV)
    Bt = (torch.eye(T, device=DEV) + 0.2).expand(B, T, T).contiguous()
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_task_diag_descriptor(x, theta, 3, Bt)
    assert desc.kind == _hip.LO_OP_KERNEL_TASK_DIAG and desc.n2 == 3 and desc.R == D and desc.N == N
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_task_mv(x, x, theta, Bt, 3, v))
    y.fill_(-7.0)
    null = ctypes.cast(None, ctypes.POINTER(_hip.OpDesc))
    checks = (("n2", 4, -1), ("n2", -1, -1), ("nterms", 0, -1), ("A0", None, -1), ("A1", None, -1), ("terms", null, -1),
              ("R", 0, -1), ("R", 32, _hip.LO_ERR_UNSUPPORTED), ("nterms", 9, _hip.LO_ERR_UNSUPPORTED))
    for field, val, rc in checks:
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_task_diag_descriptor(torch.zeros(1, 10, 33, device=DEV), torch.ones(1, 33, device=DEV), 0, Bt) is None
    assert K.kernel_task_diag_descriptor(x, theta, 0, torch.eye(9, device=DEV).expand(1, 9, 9)) is None
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
    for field, val, rc in checks:
        s = desc.c_struct()
        setattr(s, field, val)
        assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed,
                                       st) == _hip.LO_ERR_UNSUPPORTED
    y64 = torch.empty(B, N, c, dtype=torch.float64, device=DEV)
    assert lib.lo_matvec_f64(ctypes.byref(s), p(v.double()), p(y64), c, p(ws), need, st) < 0
    # the float64 CG multiplies by a descriptor through lo_matvec_desc_cb_f64, which refuses this one, and the Python
    # lowering for the float64 solvers never hands the kind over
    ctx = _hip.F64OpCtx(ctypes.pointer(s), p(ws), need)
    assert lib.lo_matvec_desc_cb_f64(ctypes.byref(ctx), p(v.double()), p(y64), B, N, c, st) != 0
    import importlib

    assert _hip.LO_OP_KERNEL_TASK_DIAG not in importlib.import_module("linear_operator_amd.utils.linear_cg")._F64_KINDS
    # not a term of LO_OP_SUM, not a base of LO_OP_MASKED
    sneed = lib.lo_matvec_workspace_bytes(ctypes.byref(both), c) + need
    sws = torch.empty(sneed, dtype=torch.uint8, device=DEV)
    assert lib.lo_matvec_f32(ctypes.byref(both), p(v), p(y), c, p(sws), sneed, st) == -1
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(both), *args) == -1
    idx = torch.arange(0, N, 2, device=DEV)
    assert K.masked_descriptor(desc, idx) is None
    masked = K.OperatorDescriptor(_hip.LO_OP_MASKED, B, idx.numel(), mask=(desc, idx)).c_struct()
    vm, ym = torch.randn(B, idx.numel(), c, device=DEV), torch.full((B, idx.numel(), c), -7.0, device=DEV)
    assert lib.lo_matvec_f32(ctypes.byref(masked), p(vm), p(ym), c, p(sws), sneed, st) == _hip.LO_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((ym == -7.0).all())


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g43_kernel_task_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in GRAD_NAMES:
            t[k].requires_grad_(True)
    return t


def task_op(p, t, guard=True):
    fn = task_fn(CASES[p][0])
    return KernelLinearOperator(t["x"], t["x"], guarded(fn, CASES[p][2]) if guard else fn, num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"], task_covar=t["task_covar"])


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_task {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(task_op(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(TaskKernel + Diag) under the reference run's solver settings, covar_func guarded against any dense evaluation:
    the descriptor kind (solve and inv_quad_logdet lower to it, not to LO_OP_CALLBACK: no closure reaches the solvers),
    the product, the diagonal, solve, inv_quad_logdet with injected probes, the pivoted Cholesky, backward."""
    G = golden(p)
    family, B, n, D, T, ard, seed = CASES[p]
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = task_op(p, t)
        assert S._native_task_refusal() is None and S._is_native_task() and not S._is_native()
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_TASK_DIAG and desc.kernel_terms == T and desc.diag_mode == 1
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.A1.shape == (B, D + 1) and (desc.N, desc.R) == (n, D)
        assert desc.task.data_ptr() == t["task_covar"].data_ptr()
        const = AddedDiagLinearOperator(S, ConstantDiagLinearOperator(t["noise"][:, :1], n))._kernel_descriptor()
        assert const.kind == _hip.LO_OP_KERNEL_TASK_DIAG and const.diag_mode == 2
        check(G, p, "mv", S @ t["V"])
        check(G, p, "mv", S.mT @ t["V"])  # (a symmetric table: the transpose is the operator itself)
        check(G, p, "mv", K.kernel_task_mv(desc.A0, desc.A0, desc.A1, desc.task, desc.n2, t["V"]))
        check(G, p, "diag", S.diagonal())
        # the solvers get the descriptor: a product through Python (the callback route of the parent) would call
        # K.kernel_task_mv from `_matmul`
        with mock.patch.object(K, "kernel_task_mv", side_effect=AssertionError("Python product")), \
                mock.patch.object(K, "pivoted_cholesky_generic", side_effect=AssertionError("row fetch")):
            check(G, p, "solve", A.solve(t["rhs"]))
            iq, ld = probed(p, t).inv_quad_logdet(t["rhs"], logdet=True)
            L, piv = S.pivoted_cholesky(RANK, return_pivots=True)
            L2, piv2 = S.pivoted_cholesky(RANK, return_pivots=True)
        check(G, p, "iq", iq)
        check(G, p, "ld", ld)
        assert np.array_equal(piv[..., :RANK].cpu().numpy(), G["piv"])
        check(G, p, "L", L)
        assert torch.equal(L, L2) and torch.equal(piv, piv2)
        # slices stay operators over the sliced points and evaluate only what is requested
        sub = S[..., 3:40, 17:90]
        assert isinstance(sub, KernelLinearOperator) and sub._is_native_task()
        names = ("x", "x", "lengthscale", "outputscale", "task_covar")
        dense64 = task_fn(family)(*(t[k].double() for k in names))[:, 3:40, 17:90]
        dense32 = task_fn(family)(*(t[k] for k in names))[:, 3:40, 17:90]
        want = host(dense64 @ t["V"][:, 17:90].double())
        within(f"{p} slice", rel(host(sub @ t["V"][:, 17:90]), want), rel(host(dense32 @ t["V"][:, 17:90]), want))
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(task_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    check(G, p, "gl", tg["lengthscale"].grad)
    check(G, p, "go", tg["outputscale"].grad)
    check(G, p, "gx", tg["x"].grad)
    check(G, p, "gB", tg["task_covar"].grad)
    assert not tg["x"].grad[..., D].any()


@pytest.mark.parametrize("p", list(CASES))
def test_gradients_through_inv_quad_against_fp64_autograd(p):
    """Lengthscale, outputscale, points and task_covar through inv_quad of TaskKernel + Diag on the matrix-free route,
    against float64 autograd on the dense matrix; the bound from the float32 run of the same computation (inv_quad under
    the same settings, autograd through the covariance function) on the STORED dense operator."""
    fn = task_fn(CASES[p][0])
    x = inputs(p)

    def leaves(dtype):
        t = {k: dev(v, dtype) for k, v in x.items()}
        for k in GRAD_NAMES:
            t[k].requires_grad_(True)
        return t

    def dense(t):
        return fn(t["x"], t["x"], t["lengthscale"], t["outputscale"], t["task_covar"])

    t64 = leaves(torch.float64)
    A64 = dense(t64) + torch.diag_embed(t64["noise"])
    (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum().backward()
    with solver_settings(settings):
        ts = leaves(torch.float32)
        AddedDiagLinearOperator(DenseLinearOperator(dense(ts)), DiagLinearOperator(ts["noise"])).inv_quad(ts["rhs"]).sum().backward()
        tg = leaves(torch.float32)
        AddedDiagLinearOperator(task_op(p, tg), DiagLinearOperator(tg["noise"])).inv_quad(tg["rhs"]).sum().backward()
    for k in GRAD_NAMES:
        want = host(t64[k].grad)
        within(f"inv_quad gradient {p} {k}", rel(host(tg[k].grad), want), rel(host(ts[k].grad), want))


def test_product_never_holds_the_matrix():
    """n = 16384, one column: the stored K would be 1 GiB.  The allocator's peak grows by at most the sizer's bytes plus
    three copies of y, through the entry point and through the operator."""
    n, D, T, c = 16384, 4, 4, 1
    g = torch.Generator().manual_seed(9970)
    x = torch.cat((torch.rand(1, n, D, generator=g), torch.randint(0, T, (1, n, 1), generator=g).float()), -1).to(DEV)
    ls, os_ = torch.full((1, 1, D), 0.3, device=DEV), torch.full((1,), 1.2, device=DEV)
    Bt = (torch.eye(T) + 0.2 * torch.rand(T, T, generator=g))
    Bt = (0.5 * (Bt + Bt.mT)).to(DEV)[None]
    v = torch.randn(1, n, c, generator=g).to(DEV)
    noise = (0.1 + torch.rand(1, n, generator=g)).to(DEV)
    theta = K.kernel_theta(ls, os_, (1,), D)
    allowed = _hip.load().lo_kernel_task_mv_workspace_bytes(1, n, n, D, T, c) + 3 * v.numel() * 4
    assert allowed < (n * n * 4) // 256
    kern = KernelLinearOperator(x, x, guarded(covariance.rbf_task, n), num_nonbatch_dimensions=NB, lengthscale=ls,
                                outputscale=os_, task_covar=Bt)
    A = AddedDiagLinearOperator(kern, DiagLinearOperator(noise))
    outs = []
    for label, call in (("entry", lambda: K.kernel_task_mv(x, x, theta, Bt, 0, v, noise)), ("kind", lambda: A._matmul(v))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs.append(call())
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
        print(f"kernel_task_mv n={n} T={T} {label}: peak growth {growth} bytes, allowed {allowed}")
        assert growth <= allowed, (label, growth, allowed)
    assert torch.equal(outs[0], outs[1])
    rows = covariance.rbf_task(x[0, :2].double(), x[0].double(), ls[0].double(), os_[0].double(), Bt[0].double())  # [2, n]
    want = rows @ v[0].double() + noise[0, :2, None].double() * v[0, :2].double()
    assert rel(host(outs[0][0, :2]), host(want)) <= 1e-5
