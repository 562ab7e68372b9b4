"""The matrix-free RBF gradient kernel (a GP with derivative observations) on the MI355X: lo_kernel_grad_mv_f32 and
lo_kernel_grad_bilinear_f32 (csrc/lo_kernel_grad.hip) against the float64 dense matrix of covariance.rbf_grad, the kind
LO_OP_KERNEL_GRAD_DIAG through the public API (product, solve, inv_quad_logdet, pivoted Cholesky, gradients) against the
reference's goldens (tests/golden/g41_kernel_grad_*.npz), through lo_matvec_f32, CG, Lanczos and MINRES, its error codes
and refusals, and its memory.

Bounds: the protocol of tests/test_gpu_kernel_op.py / test_gpu_kernel_kron.py.  Golden quantities: the error against the
fixture's float64 value is at most REF_FACTOR = 4 times the reference's own recorded float32 error (floored at
ERR_FLOOR = 1e-7).  The direct entry points: 4 times the error of the torch float32 dense composition (the block matrix
formed densely, one matmul -- for the derivative: float32 autograd through it) on the same inputs, same floor.  Gradients
through inv_quad: 4 times the error of the float32 run of the same computation on the STORED dense operator.  Every test
prints the ratio it measured (DESIGN.md section 6o holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_grad import CASES, ERR_FLOOR, GRAD_NAMES, PROBES, RANK, inputs, rel, solver_settings  # noqa: E402
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
RBF = _hip.LO_KERNEL_RBF


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_grad {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def guarded(n):
    """rbf_grad failing on any dense evaluation: both arguments with all n points."""
    def covar(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError(f"covar_func was evaluated densely: {tuple(x1.shape)} x {tuple(x2.shape)}")
        return covariance.rbf_grad(x1, x2, **params)

    covar.native_family, covar.native_outputs = RBF, "grad"
    return covar


def make_inputs(seed, B, M, N, D, c, ard=True, kind="plain"):
    """Points (x2 is x1 when M == N), hyperparameters, columns and a full diagonal that differs per row."""
    g = rng(seed)
    x1 = g.random((B, M, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with u = 0 off the diagonal
        x1[:, 1::2] = x1[:, : x1[:, 1::2].shape[1] * 2: 2]
    if kind == "far":  # separations of thousands of lengthscales: every off-diagonal block underflows to 0
        x1 = (x1 * 4000.0).astype(np.float32)
        x1[:, :, 0] += 4000.0 * np.arange(M, dtype=np.float32)[None, :]
    x2 = x1 if M == N else g.random((B, N, D)).astype(np.float32)
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    v = g.standard_normal((B, N * (D + 1), c)).astype(np.float32)
    d = (0.05 + g.random((B, M * (D + 1)))).astype(np.float32)
    return x1, x2, ls, os_, v, d


def composition(x1, x2, ls, os_, v, d, diag, dtype):
    """K v + d o v with the block matrix stored densely, in `dtype` on the device."""
    y = covariance.rbf_grad(dev(x1, dtype), dev(x2, dtype), dev(ls, dtype), dev(os_, dtype)) @ dev(v, dtype)
    if diag == "full":
        y = y + dev(d, dtype)[:, :, None] * dev(v, dtype)
    elif diag == "const":
        y = y + dev(d[:, :1], dtype)[:, :, None] * dev(v, dtype)
    return y


def direct(x1, x2, ls, os_, v, d, diag):
    B, M, D = x1.shape
    theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
    dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
    tx1 = dev(x1)
    return K.kernel_grad_mv(tx1, tx1 if x2 is x1 else dev(x2), theta, RBF, dev(v), dd, const_diag=diag == "const")


# (B, M, N, D, c, diagonal): n of {1, 130, 257} (one thread, a ragged tile, a ragged second row block), D of
# {1, 3, 4, 5, 8, 9, 16} (both sides of every padded dimension), c of {1, 2, 5, 17} (every column chunk, several sweeps with a
# ragged tail), every diagonal mode, rectangular M != N, split and unsplit points, ARD and (odd positions) shared lengthscale
DIRECT_CASES = [
    (3, 257, 257, 3, 1, "full"),
    (1, 130, 130, 1, 2, "const"),
    (1, 257, 257, 4, 5, "none"),
    (2, 130, 130, 5, 17, "full"),
    (1, 257, 257, 8, 2, "full"),
    (1, 130, 130, 9, 5, "const"),
    (1, 257, 257, 16, 17, "full"),
    (1, 1, 1, 1, 1, "none"),
    (1, 1, 1, 16, 1, "full"),
    (512, 40, 40, 2, 2, "full"),
    (512, 40, 40, 2, 2, "const"),
    (2, 130, 257, 3, 5, "none"),
    (1, 257, 130, 9, 1, "none"),
    (1, 257, 1, 16, 2, "none"),
    (1, 130, 130, 8, 17, "none"),
    (3, 257, 257, 3, 1, "const"),
    (3, 257, 257, 3, 1, "none"),
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_direct_entry_point_against_the_fp64_dense_matrix(case):
    B, M, N, D, c, diag = case
    i = DIRECT_CASES.index(case)
    x1, x2, ls, os_, v, d = make_inputs(9100 + i, B, M, N, D, c, ard=i % 2 == 0)
    lib = _hip.load()
    assert (lib.lo_kernel_grad_mv_workspace_bytes(B, M, N, D, c) == 256) == (B == 512 or N <= 128)  # (no split)
    want = host(composition(x1, x2, ls, os_, v, d, diag, torch.float64))
    comp = host(composition(x1, x2, ls, os_, v, d, diag, torch.float32))
    y = direct(x1, x2, ls, os_, v, d, diag)
    assert y.shape == (B, M * (D + 1), c) and torch.isfinite(y).all()
    within("mv " + "-".join(str(a) for a in case), rel(host(y), want), rel(comp, want))
    if M == N:  # the kind through lo_matvec_f32 runs the same kernel: the same bits
        theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
        dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
        desc = K.kernel_grad_diag_descriptor(dev(x1), theta, RBF, dd, const_diag=diag == "const")
        assert desc.kind == _hip.LO_OP_KERNEL_GRAD_DIAG and desc.N == M * (D + 1) and desc.R == D and desc.kernel_terms == 0
        assert torch.equal(K.matvec(desc, dev(v)), y)


@pytest.mark.parametrize("kind", ["dup", "far"])
def test_direct_entry_point_with_coincident_and_with_far_points(kind):
    B, n, D, c = 1, 130, 3, 5
    x1, x2, ls, os_, v, d = make_inputs(9200, B, n, n, D, c, kind=kind)
    want = host(composition(x1, x2, ls, os_, v, d, "full", torch.float64))
    comp = host(composition(x1, x2, ls, os_, v, d, "full", torch.float32))
    y = direct(x1, x2, ls, os_, v, d, "full")
    assert torch.isfinite(y).all()
    within(f"mv {kind}", rel(host(y), want), rel(comp, want))
    if kind == "far":  # only the diagonal blocks survive: y[(i, a)] = os^2 (1, theta^2)[a] v[(i, a)] + d o v
        scale = np.concatenate([np.ones((B, 1)), 1.0 / ls[:, 0].astype(np.float64) ** 2], -1) * os_.astype(np.float64)[:, None] ** 2
        blocks = np.tile(scale, (1, n))[:, :, None] * v.astype(np.float64)
        assert rel(host(y), blocks + d[:, :, None].astype(np.float64) * v) <= 1e-6


@pytest.mark.parametrize("shape", [(1, 257, 8, 5), (1, 300, 16, 17), (512, 40, 2, 2)], ids=["split-d8", "split-d16", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, n, D, c = shape
    x1, x2, ls, os_, v, d = make_inputs(9300, B, n, n, D, c)
    assert (_hip.load().lo_kernel_grad_mv_workspace_bytes(B, n, n, D, c) > 256) == (B == 1)
    assert torch.equal(direct(x1, x2, ls, os_, v, d, "full"), direct(x1, x2, ls, os_, v, d, "full"))
    theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
    U = dev(rng(9301).standard_normal(v.shape).astype(np.float32))
    g1 = K.kernel_grad_bilinear(dev(x1), dev(x1), theta, RBF, U, dev(v))
    assert torch.equal(g1, K.kernel_grad_bilinear(dev(x1), dev(x1), theta, RBF, U, dev(v)))


def test_error_codes_of_the_entry_points():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, c = 1, 300, 3, 2
    N = n * (D + 1)
    x = torch.rand(B, n, D, device=DEV)
    x70 = torch.rand(B, 70, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    v = torch.randn(B, N, c, device=DEV)
    y = torch.full((B, N, c), -7.0, device=DEV)
    g = torch.full((B, D + 1), -7.0, device=DEV)
    dfull = torch.ones(B, N, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_grad_mv_workspace_bytes(B, n, n, D, c)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    bneed = lib.lo_kernel_grad_bilinear_workspace_bytes(B, n, n, D, c)
    bws = torch.empty(bneed, dtype=torch.uint8, device=DEV)

    def mv(xa=x, xb=x, th=theta, fam=0, b=B, m=n, nn=n, dim=D, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_grad_mv_f32(p(xa), p(xb), p(th), fam, b, m, nn, dim, p(vv), cc, p(dd), mode, p(yy), p(w), wb, st)

    def bil(xa=x, xb=x, th=theta, fam=0, b=B, m=n, nn=n, dim=D, uu=v, vv=v, tt=c, gg=g, w=bws, wb=bneed):
        return lib.lo_kernel_grad_bilinear_f32(p(xa), p(xb), p(th), fam, b, m, nn, dim, p(uu), p(vv), tt, p(gg), p(w), wb, st)

    assert mv() == 0 and mv(dd=dfull, mode=1) == 0 and mv(dd=dfull, mode=2) == 0 and bil() == 0
    torch.cuda.synchronize()
    y.fill_(-7.0)
    g.fill_(-7.0)
    for bad in (dict(xa=None), dict(xb=None), dict(th=None), dict(vv=None), dict(yy=None), dict(b=0), dict(m=0), dict(nn=0),
                dict(nn=-1), dict(dim=0), dict(cc=0), dict(fam=4), dict(fam=-1), dict(mode=1), dict(mode=2), dict(mode=3),
                dict(xb=x70, nn=70, dd=dfull, mode=1), dict(xb=x70, nn=70, dd=dfull, mode=2)):  # (d only when M == N)
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    for bad in (dict(xa=None), dict(xb=None), dict(th=None), dict(uu=None), dict(vv=None), dict(gg=None), dict(b=0),
                dict(m=0), dict(nn=0), dict(dim=0), dict(tt=0), dict(fam=4), dict(fam=-1)):
        assert bil(**bad) == -1, bad
    for fam in (1, 2, 3):  # a Matern family: a valid code the gradient kernel is not built for
        assert mv(fam=fam) == _hip.LO_ERR_UNSUPPORTED and bil(fam=fam) == _hip.LO_ERR_UNSUPPORTED
    wide, th17 = torch.rand(1, 10, 17, device=DEV), torch.ones(1, 18, device=DEV)
    v180, y180 = torch.randn(1, 180, 1, device=DEV), torch.full((1, 180, 1), -7.0, device=DEV)
    assert mv(xa=wide, xb=wide, th=th17, m=10, nn=10, dim=17, vv=v180, cc=1, yy=y180) == _hip.LO_ERR_UNSUPPORTED
    assert bil(xa=wide, xb=wide, th=th17, m=10, nn=10, dim=17, uu=v180, vv=v180, tt=1) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_kernel_grad_mv_workspace_bytes(1, 10, 10, 17, 1) == 0
    # a short workspace is refused before anything is launched: y and g keep their fill (as after every refusal above)
    assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3 and bil(wb=bneed - 1) == -3 and bil(w=None, wb=0) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((y180 == -7.0).all()) and bool((g == -7.0).all())


def test_error_codes_and_refusals_of_the_kind():
    """LO_OP_KERNEL_GRAD_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; the float64
    entry points, the resident engines, the fused solve and the solve sessions refuse the kind, a sum does not take it as
    a term and a mask not as its base."""
    lib, p = _hip.load(), _hip.ptr
    B, n, D, c = 1, 150, 3, 2
    N = n * (D + 1)
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_grad_diag_descriptor(x, theta, RBF)
    assert desc.kind == _hip.LO_OP_KERNEL_GRAD_DIAG and desc.n2 == 0 and desc.R == D and desc.N == N
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_grad_mv(x, x, theta, RBF, v))
    y.fill_(-7.0)
    checks = (("n2", 4, -1), ("n2", -1, -1), ("N", N + 1, -1), ("A0", None, -1), ("A1", None, -1), ("R", 0, -1),
              ("n2", 3, _hip.LO_ERR_UNSUPPORTED), ("n2", 1, _hip.LO_ERR_UNSUPPORTED))
    for field, val, rc in checks:
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, val)
    s = desc.c_struct()
    s.R, s.N = 17, 18 * 10  # (N % (R + 1) == 0, D beyond LO_KERNEL_GRAD_MAX_DIM)
    assert run() == _hip.LO_ERR_UNSUPPORTED
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_grad_diag_descriptor(torch.rand(1, 10, 17, device=DEV), torch.ones(1, 18, device=DEV), RBF) is None
    assert K.kernel_grad_diag_descriptor(x, theta, _hip.LO_KERNEL_MATERN52) is None
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
    # the solver engines: with a preconditioner of rank 5 the plan names no resident engine, the one-launch fused solve
    # does not take the kind and no session is created for it
    noise = torch.full((B, N), 0.5, device=DEV)
    full = K.kernel_grad_diag_descriptor(x, theta, RBF, noise)
    Lp, _ = K.pivoted_cholesky(full.without_diag(), 5)
    pre = K.precond_build(Lp, noise, constant_diag=False)
    plan = K.cg_plan(full, 1, precond=pre)
    assert not plan["resident"] and plan["serial_engine"] == "none" and plan["rspace"] == "none" and plan["lockstep_cols"] == 0
    prm = K._cg_params(1, 0, 1000, 20, 1.0, 1e-10, 1e-10, 0)
    fs = full.c_struct()
    assert not lib.lo_solve_fused_supported(ctypes.byref(fs), 5, ctypes.byref(prm))
    live = K.cg_sessions_live()
    assert K._CgSession(lib, full, pre, prm, v.device).handle is None and K.cg_sessions_live() == live


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g41_kernel_grad_{p}.npz"))


def tensors(p, grad=False, dtype=torch.float32):
    t = {k: dev(v, dtype) for k, v in inputs(p).items()}
    if grad:
        for k in GRAD_NAMES:
            t[k].requires_grad_(True)
    return t


def grad_op(p, t, guard=True):
    B, n, D, seed = CASES[p]
    return KernelLinearOperator(t["x"], t["x"], guarded(n) if guard else covariance.rbf_grad,
                                num_outputs_per_input=(D + 1, D + 1), num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"])


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_grad {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(grad_op(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(GradKernel + Diag) under the reference run's solver settings, covar_func guarded against any dense evaluation: the
    descriptor kind (solve and inv_quad_logdet lower to it, not to LO_OP_CALLBACK: no closure reaches the solvers), the
    product, the diagonal, solve, inv_quad_logdet with injected probes, the pivoted Cholesky, backward."""
    G = golden(p)
    B, n, D, seed = CASES[p]
    N = n * (D + 1)
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = grad_op(p, t)
        assert S._native_grad_refusal() is None and S._native_refusal() == "more than one output per input"
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_GRAD_DIAG and desc.diag_mode == 1 and desc.N == N and desc.R == D
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.A1.shape == (B, D + 1)
        const = AddedDiagLinearOperator(S, ConstantDiagLinearOperator(t["noise"][:, :1], N))._kernel_descriptor()
        assert const.kind == _hip.LO_OP_KERNEL_GRAD_DIAG and const.diag_mode == 2
        check(G, p, "mv", S @ t["V"])
        check(G, p, "mv", K.kernel_grad_mv(desc.A0, desc.A0, desc.A1, desc.n2, t["V"]))
        check(G, p, "diag", S.diagonal())
        # the solvers get the descriptor: a product through Python (the callback route of the parent) would call
        # K.kernel_grad_mv, a row fetch K.pivoted_cholesky_generic
        with mock.patch.object(K, "kernel_grad_mv", side_effect=AssertionError("Python product")), \
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
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(grad_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    check(G, p, "gl", tg["lengthscale"].grad)
    check(G, p, "go", tg["outputscale"].grad)


@pytest.mark.parametrize("p", list(CASES))
def test_gradients_through_inv_quad_against_fp64_autograd(p):
    """Lengthscale and outputscale through inv_quad of GradKernel + Diag on the matrix-free route, against float64 autograd
    on the dense matrix; the bound from the float32 run of the same computation (inv_quad under the same settings, autograd
    through the covariance function) on the STORED dense operator."""
    fn = covariance.rbf_grad

    t64 = tensors(p, grad=True, dtype=torch.float64)
    A64 = fn(t64["x"], t64["x"], t64["lengthscale"], t64["outputscale"]) + torch.diag_embed(t64["noise"])
    (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum().backward()
    with solver_settings(settings):
        ts = tensors(p, grad=True)
        stored = fn(ts["x"], ts["x"], ts["lengthscale"], ts["outputscale"])
        AddedDiagLinearOperator(DenseLinearOperator(stored), DiagLinearOperator(ts["noise"])).inv_quad(ts["rhs"]).sum().backward()
        tg = tensors(p, grad=True)
        with mock.patch.object(K, "kernel_grad_bilinear", wraps=K.kernel_grad_bilinear) as native:
            AddedDiagLinearOperator(grad_op(p, tg), DiagLinearOperator(tg["noise"])).inv_quad(tg["rhs"]).sum().backward()
        assert native.call_count >= 1
    for k in GRAD_NAMES:
        want = host(t64[k].grad)
        within(f"inv_quad gradient {p} {k}", rel(host(tg[k].grad), want), rel(host(ts[k].grad), want))


# (B, M, N, D, t, ARD): every padded dimension and its column chunk (8 / 4 / 2) with a ragged last chunk, rectangular,
# split and unsplit, a shared lengthscale (its gradient is the sum over the dimensions)
BILINEAR_CASES = [(2, 130, 130, 3, 9, True), (1, 257, 257, 4, 1, False), (1, 257, 130, 5, 5, True), (1, 130, 257, 8, 6, False),
                  (1, 257, 257, 9, 3, True), (1, 130, 130, 16, 5, True), (512, 40, 40, 2, 2, True), (1, 1, 1, 1, 1, True)]


@pytest.mark.parametrize("case", BILINEAR_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_bilinear_derivative_against_fp64_autograd(case):
    """`_bilinear_derivative` of the operator (lo_kernel_grad_bilinear_f32 and the mapping from theta to the lengthscale
    and the outputscale) against float64 autograd through the dense block matrix; the bound from float32 autograd."""
    B, M, N, D, t, ard = case
    x1, x2, ls, os_, V, _ = make_inputs(9600 + BILINEAR_CASES.index(case), B, M, N, D, t, ard=ard)
    U = rng(9700).standard_normal((B, M * (D + 1), t)).astype(np.float32)

    def dense_grads(dtype):
        l, o = dev(ls, dtype).requires_grad_(True), dev(os_, dtype).requires_grad_(True)
        Kd = covariance.rbf_grad(dev(x1, dtype), dev(x2, dtype), l, o)
        (dev(U, dtype) * (Kd @ dev(V, dtype))).sum().backward()
        return host(l.grad), host(o.grad)

    want, comp = dense_grads(torch.float64), dense_grads(torch.float32)
    tx1 = dev(x1)
    tl, to = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    S = KernelLinearOperator(tx1, tx1 if x2 is x1 else dev(x2), guarded(min(M, N)), num_outputs_per_input=(D + 1, D + 1),
                             num_nonbatch_dimensions=NB, lengthscale=tl, outputscale=to)
    assert S._native_grad_refusal() is None
    grads = S._bilinear_derivative(dev(U), dev(V))
    by_name = dict(zip(["x1", "x2"] + list(S._differentiable_kwargs), grads))
    assert by_name["x1"] is None and by_name["x2"] is None
    assert by_name["lengthscale"].shape == tl.shape and by_name["outputscale"].shape == to.shape
    within(f"bilinear {case} lengthscale", rel(host(by_name["lengthscale"]), want[0]), rel(comp[0], want[0]))
    within(f"bilinear {case} outputscale", rel(host(by_name["outputscale"]), want[1]), rel(comp[1], want[1]))


def test_points_that_ask_for_a_gradient_take_the_general_path():
    B, n, D, t = 1, 40, 3, 2
    x1, _, ls, os_, V, _ = make_inputs(9800, B, n, n, D, t)
    tx = dev(x1).requires_grad_(True)
    tl = dev(ls).requires_grad_(True)
    S = KernelLinearOperator(tx, tx, covariance.rbf_grad, num_outputs_per_input=(D + 1, D + 1), num_nonbatch_dimensions=NB,
                             lengthscale=tl, outputscale=dev(os_))
    with mock.patch.object(K, "kernel_grad_bilinear", side_effect=AssertionError("native")):
        grads = S._bilinear_derivative(dev(V), dev(V))
    x64, l64 = dev(x1, torch.float64).requires_grad_(True), dev(ls, torch.float64).requires_grad_(True)
    Kd = covariance.rbf_grad(x64, x64, l64, dev(os_, torch.float64))
    (dev(V, torch.float64) * (Kd @ dev(V, torch.float64))).sum().backward()
    assert rel(host(grads[0] + grads[1]), host(x64.grad)) < 1e-4
    by_name = dict(zip(S._differentiable_kwargs, grads[2:]))
    assert rel(host(by_name["lengthscale"]), host(l64.grad)) < 1e-4


def test_operator_routes_and_the_kind_through_the_solvers():
    """`_matmul` and `_t_matmul` of a rectangular operator (prediction), a batch of right-hand sides broadcast over the
    operator, and the descriptor through lo_matvec_f32, the streaming CG, Lanczos and MINRES against the same entry point
    on the STORED dense matrix."""
    B, M, N, D, c = 2, 130, 70, 3, 5
    x1, x2, ls, os_, v, _ = make_inputs(9900, B, M, N, D, c)
    t1, t2 = dev(x1), dev(x2)
    S = KernelLinearOperator(t1, t2, guarded(70), num_outputs_per_input=(D + 1, D + 1), num_nonbatch_dimensions=NB,
                             lengthscale=dev(ls), outputscale=dev(os_))
    assert S._native_grad_refusal() is None and S._kernel_descriptor() is None  # (two point tensors: no square kind)
    K64 = covariance.rbf_grad(dev(x1, torch.float64), dev(x2, torch.float64), dev(ls, torch.float64), dev(os_, torch.float64))
    K32 = covariance.rbf_grad(t1, t2, dev(ls), dev(os_))
    want = host(K64 @ dev(v, torch.float64))
    within("_matmul rectangular", rel(host(S._matmul(dev(v))), want), rel(host(K32 @ dev(v)), want))
    u = dev(rng(9901).standard_normal((B, M * (D + 1), 2)).astype(np.float32))
    want = host(K64.mT @ u.double())
    within("_t_matmul rectangular", rel(host(S._t_matmul(u)), want), rel(host(K32.mT @ u), want))
    vec = dev(v[0, :, 0])  # a vector broadcast over the batch of the operator
    want = host(K64 @ vec.double())
    within("_matmul vector", rel(host(S._matmul(vec)), want), rel(host(K32 @ vec), want))
    # the square kind
    n = 257
    x, _, ls, os_, rhs, noise = make_inputs(9902, 1, n, n, D, 3)
    noise = noise * 0.2 + 0.05
    tx = dev(x)
    theta = K.kernel_theta(dev(ls), dev(os_), (1,), D)
    desc = K.kernel_grad_diag_descriptor(tx, theta, RBF, dev(noise))
    Kd = covariance.rbf_grad(tx, tx, dev(ls), dev(os_))
    dense = K.dense_diag_descriptor(Kd, dev(noise))
    A64 = covariance.rbf_grad(dev(x, torch.float64), dev(x, torch.float64), dev(ls, torch.float64),
                              dev(os_, torch.float64)) + torch.diag_embed(dev(noise, torch.float64))
    want = host(torch.linalg.solve(A64, dev(rhs, torch.float64)))
    got = K.cg_solve(desc, dev(rhs), tolerance=1e-5, max_iter=2000)
    assert not K.cg_last_executed()["resident"]  # (the streaming engine served the kind)
    ref = K.cg_solve(dense, dev(rhs), tolerance=1e-5, max_iter=2000)
    within("cg", rel(host(got.x), want), rel(host(ref.x), want))
    qn, tn = K.lanczos_tridiag(desc, dev(rhs), 12)
    qd, td = K.lanczos_tridiag(dense, dev(rhs), 12)
    assert tn.shape == td.shape and rel(host(tn), host(td)) < 1e-3
    shifts = torch.tensor([0.0, 0.5], device=DEV)
    mn, md = K.minres_solve(desc, dev(rhs), shifts, max_iter=400), K.minres_solve(dense, dev(rhs), shifts, max_iter=400)
    want = np.stack([host(torch.linalg.solve(A64 + s * torch.eye(A64.shape[-1], device=DEV, dtype=torch.float64),
                                            dev(rhs, torch.float64))) for s in (0.0, 0.5)])
    within("minres", rel(host(mn.x), want), rel(host(md.x), want))


def test_product_never_holds_the_matrix():
    """n = 8192, D = 3, one column: the stored operator would be 4 GiB.  The allocator's peak grows by at most the sizer's
    bytes (the partials) plus three copies of y, through the entry point and through the operator."""
    n, D, c = 8192, 3, 1
    N = n * (D + 1)
    g = torch.Generator().manual_seed(9500)
    x = torch.rand(1, n, D, generator=g).to(DEV)
    ls, os_ = torch.tensor([[[0.3, 0.4, 0.5]]], device=DEV), torch.full((1,), 1.2, device=DEV)
    v = torch.randn(1, N, c, generator=g).to(DEV)
    noise = (0.1 + torch.rand(1, N, generator=g)).to(DEV)
    theta = K.kernel_theta(ls, os_, (1,), D)
    allowed = _hip.load().lo_kernel_grad_mv_workspace_bytes(1, n, n, D, c) + 3 * v.numel() * 4
    assert allowed < 2 ** 26
    S = KernelLinearOperator(x, x, guarded(n), num_outputs_per_input=(D + 1, D + 1), num_nonbatch_dimensions=NB,
                             lengthscale=ls, outputscale=os_)
    A = AddedDiagLinearOperator(S, DiagLinearOperator(noise))
    outs = []
    for label, call in (("entry", lambda: K.kernel_grad_mv(x, x, theta, RBF, v, noise)), ("operator", lambda: A._matmul(v))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs.append(call())
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
        print(f"kernel_grad_mv n={n} D={D} {label}: peak growth {growth} bytes, allowed {allowed}")
        assert growth <= allowed, (label, growth, allowed)
    assert torch.equal(outs[0], outs[1])
    rows = covariance.rbf_grad(x[0, :2].double(), x[0].double(), ls[0].double(), os_[0].double())  # [2 (D + 1), N]
    want = rows @ v[0].double() + noise[0, : 2 * (D + 1), None].double() * v[0, : 2 * (D + 1)].double()
    assert rel(host(outs[0][0, : 2 * (D + 1)]), host(want)) <= 1e-5
