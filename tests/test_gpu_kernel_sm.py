"""The matrix-free spectral mixture kernel on the MI355X: lo_kernel_sm_mv_f32 / lo_kernel_sm_bilinear_f32 /
lo_kernel_sm_points_grad_f32 (csrc/lo_kernel_sm.hip) against the float64 dense composition, the kind LO_OP_KERNEL_SM_DIAG
through the public API (product, diagonal, solve, inv_quad_logdet, pivoted Cholesky, gradients) against the reference's
goldens (tests/golden/g48_kernel_sm_*.npz), as a term of LO_OP_SUM, and its error codes and refusals.

Bounds: the protocol of tests/test_gpu_kernel_param.py, unchanged.  Direct entry points: the error against the float64
dense composition (for the derivatives: float64 autograd through it) is at most REF_FACTOR = 4 times the error of the torch
float32 dense composition on the same inputs, floored at ERR_FLOOR = 1e-7.  Golden quantities: 4 times the reference's own
recorded float32 error.  Every test prints the ratio it measured (DESIGN.md section 6v holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_sm import (  # noqa: E402
    CASES, ERR_FLOOR, GRADS, NB, PARAMS, PROBES, RANK, inputs, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    SumLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
SM = _hip.LO_OP_KERNEL_SM_DIAG
FN = covariance.spectral_mixture


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_sm {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def guarded(n):
    """A covar_func with the tag of spectral_mixture that fails on any dense evaluation."""
    def covar(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError(f"covar_func was evaluated densely: {tuple(x1.shape)} x {tuple(x2.shape)}")
        return FN(x1, x2, **params)

    covar.native_outputs = FN.native_outputs
    return covar


def make_inputs(seed, B, M, N, D, Q, c, span=3.0):
    """Points of both sides (one array when M == N) on [0, span]^D, the mixtures (frequencies 0.3 .. 1 cycles per unit:
    the points cover about `span` periods; bandwidths such that the envelope spans the domain), columns and a full
    diagonal."""
    g = rng(seed)
    x1 = (span * g.random((B, M, D))).astype(np.float32)
    x2 = x1 if M == N else (span * g.random((B, N, D))).astype(np.float32)
    w = (0.3 + 0.7 * g.random((B, Q))).astype(np.float32)
    mu = (0.3 + 0.7 * g.random((B, Q, D))).astype(np.float32)
    sg = ((0.1 + 0.3 * g.random((B, Q, D))) * (3.0 / span) / np.sqrt(D)).astype(np.float32)
    v = g.standard_normal((B, N, c)).astype(np.float32)
    d = (0.05 + g.random((B, N))).astype(np.float32)
    return x1, x2, w, mu, sg, v, d


def theta_of(w, mu, sg):
    return K.kernel_sm_theta(dev(w), dev(mu), dev(sg), (w.shape[0],), mu.shape[-1])


def composition(x1, x2, w, mu, sg, v, d, diag, dtype):
    """K(x1, x2) v + d o v with K stored densely, in `dtype` on the device."""
    A = FN(dev(x1, dtype), dev(x2, dtype), dev(w, dtype), dev(mu, dtype), dev(sg, dtype))
    y = A @ dev(v, dtype)
    if diag == "full":
        y = y + dev(d, dtype)[:, :, None] * dev(v, dtype)
    elif diag == "const":
        y = y + dev(d[:, :1], dtype)[:, :, None] * dev(v, dtype)
    return y


def diag_operand(d, diag):
    return None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))


def direct(x1, x2, w, mu, sg, v, d, diag):
    tx1 = dev(x1)
    tx2 = tx1 if x2 is x1 else dev(x2)
    return K.kernel_sm_mv(tx1, tx2, theta_of(w, mu, sg), dev(v), diag_operand(d, diag), const_diag=diag == "const")


def split_expected(B, M, N):
    return not (B * -(-M // 256) >= 512 or N <= 128)


# (B, M, N, D, Q, c, diagonal, span): split columns; unsplit; padded D; both limits with two column sweeps; rectangular;
# D = 1; points over more than 600 periods of the fastest mixture (the range reduction)
SHAPES = [
    (2, 300, 257, 3, 2, 3, "none", 3.0),
    (512, 130, 130, 2, 1, 1, "full", 3.0),
    (1, 140, 140, 5, 3, 4, "const", 3.0),
    (1, 140, 140, 16, 16, 17, "full", 3.0),
    (1, 70, 300, 3, 2, 17, "none", 3.0),
    (1, 257, 257, 1, 4, 1, "full", 3.0),
    (2, 257, 257, 2, 2, 3, "full", 2400.0),
]


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "-".join(str(x) for x in c))
def test_product_against_the_fp64_composition(case):
    B, M, N, D, Q, c, diag, span = case
    x1, x2, w, mu, sg, v, d = make_inputs(9600 + SHAPES.index(case), B, M, N, D, Q, c, span)
    if span > 600:  # every member's points span more than 600 periods of its fastest mixture
        assert ((x1.max(1) - x1.min(1))[:, None, :] * mu).max((1, 2)).min() > 600
    lib = _hip.load()
    assert (lib.lo_kernel_sm_mv_workspace_bytes(B, M, N, D, Q, c) > 256) == split_expected(B, M, N)
    want = host(composition(x1, x2, w, mu, sg, v, d, diag, torch.float64))
    comp = host(composition(x1, x2, w, mu, sg, v, d, diag, torch.float32))
    y = direct(x1, x2, w, mu, sg, v, d, diag)
    assert y.shape == (B, M, c) and torch.isfinite(y).all()
    within("mv " + "-".join(str(a) for a in case), rel(host(y), want), rel(comp, want))
    assert torch.equal(direct(x1, x2, w, mu, sg, v, d, diag), y)  # two calls: equal bits
    if M == N:  # the kind through lo_matvec_f32 runs the same kernel: the same bits
        theta = theta_of(w, mu, sg)
        desc = K.kernel_sm_diag_descriptor(dev(x1), theta, diag_operand(d, diag), const_diag=diag == "const")
        assert desc.kind == SM and desc.N == N and desc.R == D and desc.n2 == Q and desc.A1.shape == (B, Q, 2 * D + 1)
        assert torch.equal(K.matvec(desc, dev(v)), y)
        # the matrix read off with identity columns: K(x, y) and K(y, x) have equal bits
        eye = torch.eye(N, device=DEV).expand(B, N, N).contiguous()
        Kd = K.kernel_sm_mv(dev(x1), dev(x1), theta, eye)
        assert torch.equal(Kd, Kd.mT)


def autograd_all(x1, x2, w, mu, sg, U, V, dtype):
    """d / d (theta, x1, x2) of sum_s u_s^T K(x1, x2) v_s by torch autograd in `dtype` through the dense function, theta
    [B, Q, 2 D + 1] = (w, mu, sigma) as the leaf the entry point differentiates by."""
    D = mu.shape[-1]
    theta = torch.cat((dev(w, dtype)[..., None], dev(mu, dtype), dev(sg, dtype)), -1).requires_grad_(True)
    a, b = dev(x1, dtype).requires_grad_(True), dev(x2, dtype).requires_grad_(True)
    dense = FN(a, b, theta[..., 0], theta[..., 1:1 + D], theta[..., 1 + D:])
    (dev(U, dtype) * (dense @ dev(V, dtype))).sum().backward()
    return [host(t.grad) for t in (theta, a, b)]


# (B, M, N, D, Q, t, quarter): split and unsplit shapes with t = 1 and t = 11 (a second sweep of the 8 columns); `quarter`:
# a pair with mu tau = 1/4 exactly in every coordinate of mixture 0, where the cosine is 0 (the no-division rule)
DERIV_SHAPES = [
    (2, 300, 257, 3, 2, 1, False),
    (512, 130, 130, 2, 1, 11, False),
    (1, 140, 140, 5, 3, 11, True),
    (1, 70, 300, 16, 16, 1, False),
    (1, 257, 257, 1, 4, 11, True),
]


@pytest.mark.parametrize("case", DERIV_SHAPES, ids=lambda c: "-".join(str(x) for x in c))
def test_bilinear_and_points_gradient_against_fp64_autograd(case):
    B, M, N, D, Q, t, quarter = case
    label = "-".join(str(a) for a in case)
    x1, x2, w, mu, sg, _, _ = make_inputs(9650 + DERIV_SHAPES.index(case), B, M, N, D, Q, 1)
    g = rng(9690)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    if M == N:  # (x1 is x2 as arrays; as autograd leaves the two sides are apart, as the entry points hold them)
        x2 = x1.copy()
    if quarter:  # mu = 1/2, tau = 1/2, both exact in float32
        mu[:, 0, :] = 0.5
        x1[:, 0, :] = 1.25
        x2[:, 1, :] = 1.75
        assert np.all(mu[:, 0, :] * (x2[:, 1, :] - x1[:, 0, :]) == 0.25)
    want = autograd_all(x1, x2, w, mu, sg, U, V, torch.float64)
    ref = autograd_all(x1, x2, w, mu, sg, U, V, torch.float32)
    tx1, tx2, tU, tV = dev(x1), dev(x2), dev(U), dev(V)
    theta = theta_of(w, mu, sg)
    g_theta = K.kernel_sm_bilinear(tx1, tx2, theta, tU, tV)
    g_x1 = K.kernel_sm_points_grad(tx1, tx2, theta, tU, tV)
    g_x2 = K.kernel_sm_points_grad(tx2, tx1, theta, tV, tU)
    assert g_theta.shape == (B, Q, 2 * D + 1) and g_x1.shape == (B, M, D) and g_x2.shape == (B, N, D)
    for got in (g_theta, g_x1, g_x2):
        assert torch.isfinite(got).all()
    for what, got, wnt, r in (("weights", g_theta[..., 0], want[0][..., 0], ref[0][..., 0]),
                              ("means", g_theta[..., 1:1 + D], want[0][..., 1:1 + D], ref[0][..., 1:1 + D]),
                              ("scales", g_theta[..., 1 + D:], want[0][..., 1 + D:], ref[0][..., 1 + D:]),
                              ("x1", g_x1, want[1], ref[1]), ("x2", g_x2, want[2], ref[2])):
        within(f"{what} {label}", rel(host(got), wnt), rel(r, wnt))
    # two calls give the same bits
    assert torch.equal(K.kernel_sm_bilinear(tx1, tx2, theta, tU, tV), g_theta)
    assert torch.equal(K.kernel_sm_points_grad(tx1, tx2, theta, tU, tV), g_x1)


# ---------------------------------------------------------------------------------- error codes
def test_error_codes_of_the_entry_points():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, Q, c = 1, 300, 3, 2, 2
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, Q, 2 * D + 1, device=DEV)
    v = torch.randn(B, n, c, device=DEV)
    y = torch.full((B, n, c), -7.0, device=DEV)
    gt, gx = torch.full((B, Q, 2 * D + 1), -7.0, device=DEV), torch.full((B, n, D), -7.0, device=DEV)
    dfull = torch.ones(B, n, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = max(lib.lo_kernel_sm_mv_workspace_bytes(B, n, n, D, Q, c), lib.lo_kernel_sm_bilinear_workspace_bytes(B, n, n, D, Q, c),
               lib.lo_kernel_sm_points_grad_workspace_bytes(B, n, n, D, Q, c))
    assert lib.lo_kernel_sm_mv_workspace_bytes(B, n, n, D, Q, c) > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(xx=x, th=theta, q=Q, b=B, m=n, nn=n, dim=D, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_sm_mv_f32(p(xx), p(xx), p(th), q, b, m, nn, dim, p(vv), cc, p(dd), mode, p(yy), p(w), wb, st)

    def bil(xx=x, th=theta, q=Q, b=B, m=n, nn=n, dim=D, uu=v, vv=v, cc=c, g1=gt, w=ws, wb=need):
        return lib.lo_kernel_sm_bilinear_f32(p(xx), p(xx), p(th), q, b, m, nn, dim, p(uu), p(vv), cc, p(g1), p(w), wb, st)

    def pg(xx=x, th=theta, q=Q, b=B, m=n, nn=n, dim=D, uu=v, vv=v, cc=c, g1=gx, w=ws, wb=need):
        return lib.lo_kernel_sm_points_grad_f32(p(xx), p(xx), p(th), q, b, m, nn, dim, p(uu), p(vv), cc, p(g1), p(w), wb, st)

    assert mv() == 0 and mv(dd=dfull, mode=1) == 0 and mv(dd=dfull, mode=2) == 0 and bil() == 0 and pg() == 0
    torch.cuda.synchronize()
    for t in (y, gt, gx):
        t.fill_(-7.0)
    shared = (dict(xx=None), dict(th=None), dict(vv=None), dict(b=0), dict(m=0), dict(nn=0), dict(nn=-1), dict(dim=0),
              dict(cc=0), dict(q=0), dict(q=-1))
    y130 = torch.full((B, 130, c), -7.0, device=DEV)
    for bad in shared + (dict(yy=None), dict(mode=1), dict(mode=2), dict(mode=3), dict(m=130, yy=y130, dd=dfull, mode=1),
                         dict(m=130, yy=y130, dd=dfull, mode=2)):  # (a diagonal on a rectangular product)
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    for bad in shared + (dict(uu=None), dict(g1=None)):
        assert bil(**bad) == -1, bad
        assert pg(**bad) == -1, bad
    wide, th17 = torch.zeros(1, 10, 17, device=DEV), torch.ones(1, 17, 35, device=DEV)
    v10 = torch.randn(1, 10, 1, device=DEV)
    y10, gx17, gt17 = (torch.full(s, -7.0, device=DEV) for s in ((1, 10, 1), (1, 10, 17), (1, 17, 35)))
    for fn_, extra in ((mv, dict(yy=y10)), (bil, dict(uu=v10, g1=gt17)), (pg, dict(uu=v10, g1=gx17))):
        assert fn_(xx=wide, th=th17, q=2, m=10, nn=10, dim=17, vv=v10, cc=1, **extra) == _hip.LO_ERR_UNSUPPORTED  # (D = 17)
        assert fn_(th=th17, q=17) == _hip.LO_ERR_UNSUPPORTED  # (Q = 17)
        assert fn_(b=65536) == _hip.LO_ERR_UNSUPPORTED  # (refused before anything is read)
        assert fn_(q=0, b=65536) == -1  # (Q < 1 is a bad argument, checked first)
    # a short workspace is refused before anything is launched: the outputs keep their fill (as after every refusal above)
    assert mv(wb=lib.lo_kernel_sm_mv_workspace_bytes(B, n, n, D, Q, c) - 1) == -3 and mv(w=None, wb=0) == -3
    assert bil(wb=255) == -3 and bil(w=None, wb=0) == -3 and pg(wb=255) == -3 and pg(w=None, wb=0) == -3
    torch.cuda.synchronize()
    for t in (y, gt, gx, y10, y130, gx17, gt17):
        assert bool((t == -7.0).all())


def test_error_codes_and_refusals_of_the_kind():
    """LO_OP_KERNEL_SM_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; a term of
    LO_OP_SUM; the float64 entry points and a mask refuse the kind."""
    lib, p = _hip.load(), _hip.ptr
    B, N, D, Q, c = 1, 300, 3, 2, 2
    x = torch.rand(B, N, D, device=DEV)
    theta = torch.rand(B, Q, 2 * D + 1, device=DEV) + 0.2
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_sm_diag_descriptor(x, theta)
    assert desc.kind == SM and desc.n2 == Q and desc.R == D and desc.N == N
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_sm_mv(x, x, theta, v))
    y.fill_(-7.0)
    checks = (("n2", 0, -1), ("n2", -1, -1), ("A0", None, -1), ("A1", None, -1), ("R", 0, -1),
              ("n2", 17, _hip.LO_ERR_UNSUPPORTED), ("R", 17, _hip.LO_ERR_UNSUPPORTED), ("B", 65536, _hip.LO_ERR_UNSUPPORTED))
    for field, val, rc in checks:
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_sm_diag_descriptor(torch.zeros(1, 10, 17, device=DEV), torch.ones(1, 2, 35, device=DEV)) is None
    assert K.kernel_sm_diag_descriptor(x, torch.ones(1, 17, 2 * D + 1, device=DEV)) is None
    # the pivoted Cholesky, the kind alone and as a term of a sum
    L, perm = torch.empty(B, 5, N, device=DEV), torch.empty(B, N, dtype=torch.int64, device=DEV)
    rank = ctypes.c_int32(0)
    root = K.lowrank_diag_descriptor(torch.rand(B, N, 4, device=DEV), None)
    both = K.sum_descriptor([desc, root]).c_struct()
    pneed = max(lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(s), 5),
                lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(both), 5))
    pws = torch.empty(pneed, dtype=torch.uint8, device=DEV)
    args = (5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed, st)
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == 0 and rank.value == 5
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(both), *args) == 0 and rank.value == 5
    for field, val, rc in checks[:-1]:  # (the streaming engine launches no sweep: no batch limit of its own)
        s = desc.c_struct()
        setattr(s, field, val)
        assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed,
                                       st) == _hip.LO_ERR_UNSUPPORTED
    y64 = torch.empty(B, N, c, dtype=torch.float64, device=DEV)
    assert lib.lo_matvec_f64(ctypes.byref(s), p(v.double()), p(y64), c, p(ws), need, st) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_matvec_f64(ctypes.byref(both), p(v.double()), p(y64), c, p(ws), need, st) < 0
    ctx = _hip.F64OpCtx(ctypes.pointer(s), p(ws), need)
    assert lib.lo_matvec_desc_cb_f64(ctypes.byref(ctx), p(v.double()), p(y64), B, N, c, st) != 0
    import importlib

    assert SM not in importlib.import_module("linear_operator_amd.utils.linear_cg")._F64_KINDS
    # the sum takes it as a term: the product is the terms' products added
    sneed = lib.lo_matvec_workspace_bytes(ctypes.byref(both), c)
    sws = torch.empty(sneed, dtype=torch.uint8, device=DEV)
    assert lib.lo_matvec_f32(ctypes.byref(both), p(v), p(y), c, p(sws), sneed, st) == 0
    torch.cuda.synchronize()
    want = K.kernel_sm_mv(x, x, theta, v) + K.matvec(root, v)
    assert rel(host(y), host(want)) <= 1e-6
    # not a base of LO_OP_MASKED, alone or inside a sum
    idx = torch.arange(0, N, 2, device=DEV)
    assert K.masked_descriptor(desc, idx) is None and K.masked_descriptor(K.sum_descriptor([desc, root]), idx) is None
    vm, ym = torch.randn(B, idx.numel(), c, device=DEV), torch.full((B, idx.numel(), c), -7.0, device=DEV)
    for base in (desc, K.sum_descriptor([desc, root])):
        masked = K.OperatorDescriptor(_hip.LO_OP_MASKED, B, idx.numel(), mask=(base, idx)).c_struct()
        mneed = max(lib.lo_matvec_workspace_bytes(ctypes.byref(masked), c), 1 << 20)
        mws = torch.empty(mneed, dtype=torch.uint8, device=DEV)
        assert lib.lo_matvec_f32(ctypes.byref(masked), p(vm), p(ym), c, p(mws), mneed, st) == _hip.LO_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((ym == -7.0).all())


def test_the_resident_engines_and_the_sessions_refuse_the_kind():
    """The fused solve and the solve session take low-rank operators only: lo_solve_fused_supported answers 0 and
    lo_cg_session_create_f32 LO_ERR_UNSUPPORTED (no handle) for the kind."""
    lib = _hip.load()
    N = 300
    x, noise = torch.rand(1, N, 3, device=DEV), torch.ones(1, N, device=DEV)
    desc = K.kernel_sm_diag_descriptor(x, torch.rand(1, 2, 7, device=DEV) + 0.2, noise)
    prm = K._cg_params(1, 0, 100, 20, 1.0, 1e-10, 1e-10, 0)
    s = desc.c_struct()
    assert lib.lo_solve_fused_supported(ctypes.byref(s), 5, ctypes.byref(prm)) == 0
    assert not K.solve_fused_supported(desc, 1, 5)
    L, _ = K.pivoted_cholesky(desc, 5)
    pre = K.precond_build(L, noise, constant_diag=False)
    live = K.cg_sessions_live()
    session = K._CgSession(lib, desc, pre, prm, x.device)
    assert session.handle is None and K.cg_sessions_live() == live


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g48_kernel_sm_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in GRADS.values():
            t[k].requires_grad_(True)
    return t


def sm_op(p, t, guard=True):
    return KernelLinearOperator(t["x"], t["x"], guarded(CASES[p][1]) if guard else FN, num_nonbatch_dimensions=NB,
                                **{k: t[k] for k in PARAMS})


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_sm {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(sm_op(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(SM + Diag) under the reference run's solver settings, covar_func guarded against any dense evaluation: the
    descriptor kind (solve and inv_quad_logdet lower to it, not to LO_OP_CALLBACK), the product, the diagonal, solve,
    inv_quad_logdet with injected probes, the pivoted Cholesky, backward."""
    G = golden(p)
    B, n, D, Q, seed = CASES[p]
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = sm_op(p, t)
        assert S._native_sm_refusal() is None and S._is_native_sm() and not S._is_native() and not S._is_native_param()
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == SM and desc.diag_mode == 1 and desc.n2 == Q
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.A1.shape == (B, Q, 2 * D + 1) and (desc.N, desc.R) == (n, D)
        const = AddedDiagLinearOperator(S, ConstantDiagLinearOperator(t["noise"][:, :1], n))._kernel_descriptor()
        assert const.kind == SM and const.diag_mode == 2
        check(G, p, "mv", S @ t["V"])
        check(G, p, "mv", S.mT @ t["V"])
        check(G, p, "mv", K.kernel_sm_mv(desc.A0, desc.A0, desc.A1, t["V"]))
        check(G, p, "diag", S.diagonal())
        # the solvers get the descriptor: a product through Python (the callback route) would call K.kernel_sm_mv
        with mock.patch.object(K, "kernel_sm_mv", side_effect=AssertionError("Python product")), \
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
        sub = S[..., 3:40, 17:90]  # slices stay operators over the sliced points: the rectangular product
        assert isinstance(sub, KernelLinearOperator) and sub._is_native_sm()
        names = ("x", "x") + PARAMS
        dense64 = FN(*(t[k].double() for k in names))[:, 3:40, 17:90]
        dense32 = FN(*(t[k] for k in names))[:, 3:40, 17:90]
        want = host(dense64 @ t["V"][:, 17:90].double())
        within(f"{p} slice", rel(host(sub @ t["V"][:, 17:90]), want), rel(host(dense32 @ t["V"][:, 17:90]), want))
        ii, jj = torch.tensor([0, 5, n - 1], device=DEV), torch.tensor([n - 1, 5, 2], device=DEV)
        bb = torch.tensor([0, B - 1, 0], device=DEV)
        picked = S[bb, ii, jj]  # single entries: covar_func on one pair each
        full64, full32 = FN(*(t[k].double() for k in names)), FN(*(t[k] for k in names))
        within(f"{p} entries", rel(host(picked), host(full64[bb, ii, jj])), rel(host(full32[bb, ii, jj]), host(full64[bb, ii, jj])))
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(sm_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    for q, name in GRADS.items():
        check(G, p, q, tg[name].grad)


def test_sm_plus_rbf_plus_noise_lowers_to_a_sum_and_solves():
    """SumLinearOperator(SM, rbf) + Diag: one LO_OP_SUM descriptor with the SM kind and the plain kernel kind as terms;
    the solve, under the reference's settings, against float64 on the stored matrix, bounded by the float32 solve of the
    STORED dense operator."""
    p = "ard"
    B, n, D, Q, seed = CASES[p]
    t = tensors(p)
    g = rng(9695)
    ls2 = dev((0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D)))).astype(np.float32))
    os2 = dev((0.5 + 0.5 * g.random(B)).astype(np.float32))

    def rbf_guard(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError("covar_func was evaluated densely")
        return covariance.rbf(x1, x2, **params)

    rbf_guard.native_family = covariance.rbf.native_family
    rbf = KernelLinearOperator(t["x"], t["x"], rbf_guard, num_nonbatch_dimensions={"outputscale": 0}, lengthscale=ls2,
                               outputscale=os2)
    S = SumLinearOperator(sm_op(p, t), rbf)
    A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
    desc = A._kernel_descriptor()
    assert desc.kind == _hip.LO_OP_SUM and desc.diag_mode == 1
    assert [term.kind for term in desc.terms] == [SM, _hip.LO_OP_KERNEL_DIAG]
    d64 = lambda a: a.double()  # noqa: E731
    dense64 = (FN(d64(t["x"]), d64(t["x"]), *(d64(t[k]) for k in PARAMS))
               + covariance.rbf(d64(t["x"]), d64(t["x"]), d64(ls2), d64(os2)))
    dense32 = FN(t["x"], t["x"], *(t[k] for k in PARAMS)) + covariance.rbf(t["x"], t["x"], ls2, os2)
    want_mv = host(dense64 @ d64(t["V"]))
    within("sum mv", rel(host(S @ t["V"]), want_mv), rel(host(dense32 @ t["V"]), want_mv))
    want = host(torch.linalg.solve(dense64 + torch.diag_embed(d64(t["noise"])), d64(t["rhs"])))
    with solver_settings(settings):
        with mock.patch.object(K, "kernel_sm_mv", side_effect=AssertionError("Python product")):
            got = A.solve(t["rhs"])
        ref = AddedDiagLinearOperator(DenseLinearOperator(dense32), DiagLinearOperator(t["noise"])).solve(t["rhs"])
    within("sum solve", rel(host(got), want), rel(host(ref), want))
