"""The matrix-free multitask operator Kron(Kernel(X, X), Dense(Bt)) on the MI355X: lo_kernel_kron_mv_f32
(csrc/lo_kernel_kron.hip) against the float64 dense composition, the kind LO_OP_KERNEL_KRON_DIAG through the public API
(product, solve, inv_quad_logdet, pivoted Cholesky, gradients) against the reference's goldens
(tests/golden/g40_kernel_kron_*.npz), its error codes and refusals, and its memory.

Bounds: the protocol of tests/test_gpu_kernel_op.py.  Golden quantities: the error against the fixture's float64 value is
at most REF_FACTOR = 4 times the reference's own recorded float32 error (floored at ERR_FLOOR = 1e-7).  The direct entry
point: 4 times the error of the torch float32 dense composition (K (x) Bt formed densely, one matmul) on the same inputs,
same floor.  Gradients through inv_quad: 4 times the error of the float32 run of the same computation on the STORED dense
operator.  Every test prints the ratio it measured (DESIGN.md section 6n holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_kron import (  # noqa: E402
    CASES, ERR_FLOOR, GRAD_NAMES, PROBES, RANK, dense_kron, inputs, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator)

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
    print(f"kernel_kron {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def guarded(fn, n):
    """A covar_func of the same native family that fails on any dense evaluation: both arguments with all n points."""
    def covar(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError(f"covar_func was evaluated densely: {tuple(x1.shape)} x {tuple(x2.shape)}")
        return fn(x1, x2, **params)

    covar.native_family = fn.native_family
    return covar


def make_inputs(seed, B, n, D, T, c, ard=True, kind="plain"):
    """Points, hyperparameters, a NON-symmetric Bt, columns and a full diagonal that differs per (i, t)."""
    g = rng(seed)
    x = g.random((B, n, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with r = 0 off the diagonal
        x[:, 1::2] = x[:, : x[:, 1::2].shape[1] * 2: 2]
    if kind == "far":  # separations of thousands of lengthscales: every off-diagonal kernel value underflows to 0
        x = (x * 4000.0).astype(np.float32)
        x[:, :, 0] += 4000.0 * np.arange(n, dtype=np.float32)[None, :]
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    Bt = (np.eye(T) * (1.0 + 0.3 * np.arange(T)) + 0.5 * (g.random((B, T, T)) - 0.3) * (1 - np.eye(T))).astype(np.float32)
    v = g.standard_normal((B, n * T, c)).astype(np.float32)
    d = (0.05 + g.random((B, n * T))).astype(np.float32)
    return x, ls, os_, Bt, v, d


def composition(fn, x, ls, os_, Bt, v, d, diag, dtype):
    """(K (x) Bt) v + d o v with the product stored densely, in `dtype` on the device."""
    A = dense_kron(fn(dev(x, dtype), dev(x, dtype), dev(ls, dtype), dev(os_, dtype)), dev(Bt, dtype))
    y = A @ dev(v, dtype)
    if diag == "full":
        y = y + dev(d, dtype)[:, :, None] * dev(v, dtype)
    elif diag == "const":
        y = y + dev(d[:, :1], dtype)[:, :, None] * dev(v, dtype)
    return y


def direct(fn, x, ls, os_, Bt, v, d, diag):
    B, n, D = x.shape
    theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
    dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
    return K.kernel_kron_mv(dev(x), theta, dev(Bt), fn.native_family, dev(v), dd, const_diag=diag == "const")


# (family, B, n, D, T, c, diagonal): every family, every padded D, T of {1, 2, 3, 8}, wide columns T c of {1, 2, 4, 24, 51}
# (every accumulator width, several sweeps with a ragged tail), one tile / a ragged tile / several tiles, split and
# unsplit points, every diagonal mode
DIRECT_CASES = [
    ("rbf", 3, 257, 3, 2, 1, "full"),
    ("matern12", 1, 63, 1, 1, 4, "const"),
    ("matern32", 1, 130, 32, 8, 3, "full"),
    ("matern52", 1, 300, 8, 3, 17, "none"),
    ("matern52", 1, 300, 8, 3, 17, "full"),
    ("rbf", 512, 40, 2, 2, 2, "const"),
    ("rbf", 512, 40, 2, 2, 2, "full"),
    ("rbf", 1, 1, 1, 1, 1, "none"),
    ("rbf", 3, 257, 3, 2, 1, "const"),
    ("rbf", 3, 257, 3, 2, 1, "none"),
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_direct_entry_point_against_the_fp64_composition(case):
    name, B, n, D, T, c, diag = case
    fn = covariance.FAMILIES[name]
    x, ls, os_, Bt, v, d = make_inputs(9100 + DIRECT_CASES.index(case), B, n, D, T, c)
    if T > 1:
        assert not np.allclose(Bt, Bt.transpose(0, 2, 1))  # (a transposed task product would not pass)
    lib = _hip.load()
    assert (lib.lo_kernel_kron_mv_workspace_bytes(B, n, D, T, c) == 256) == (B == 512 or n <= 128)  # (one tile, or workgroups enough: no split)
    want = host(composition(fn, x, ls, os_, Bt, v, d, diag, torch.float64))
    comp = host(composition(fn, x, ls, os_, Bt, v, d, diag, torch.float32))
    y = direct(fn, x, ls, os_, Bt, v, d, diag)
    assert y.shape == (B, n * T, c) and torch.isfinite(y).all()
    within("mv " + "-".join(str(a) for a in case), rel(host(y), want), rel(comp, want))
    # the kind through lo_matvec_f32 runs the same kernel: the same bits
    theta = K.kernel_theta(dev(ls), dev(os_), (B,), D)
    dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
    desc = K.kernel_kron_diag_descriptor(dev(x), theta, fn.native_family, dev(Bt), dd, const_diag=diag == "const")
    assert desc.kind == _hip.LO_OP_KERNEL_KRON_DIAG and desc.N == n * T and desc.kernel_terms == T
    assert torch.equal(K.matvec(desc, dev(v)), y)


@pytest.mark.parametrize("kind", ["dup", "far"])
def test_direct_entry_point_with_coincident_and_with_far_points(kind):
    name, B, n, D, T, c = "matern52", 1, 130, 3, 3, 4
    fn = covariance.FAMILIES[name]
    x, ls, os_, Bt, v, d = make_inputs(9200, B, n, D, T, c, kind=kind)
    want = host(composition(fn, x, ls, os_, Bt, v, d, "full", torch.float64))
    comp = host(composition(fn, x, ls, os_, Bt, v, d, "full", torch.float32))
    y = direct(fn, x, ls, os_, Bt, v, d, "full")
    assert torch.isfinite(y).all()
    within(f"mv {kind}", rel(host(y), want), rel(comp, want))
    if kind == "far":  # only the diagonal blocks survive: y[(i, t)] = os^2 sum_s Bt[t, s] v[(i, s)] + d o v
        v4 = v.reshape(B, n, T, c).astype(np.float64)
        blocks = os_.astype(np.float64)[:, None, None, None] ** 2 * np.einsum("bts,bisc->bitc", Bt.astype(np.float64), v4)
        assert rel(host(y), blocks.reshape(B, n * T, c) + d[:, :, None].astype(np.float64) * v) <= 1e-6


@pytest.mark.parametrize("shape", [(1, 300, 8, 3, 17), (512, 40, 2, 2, 2)], ids=["split", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, n, D, T, c = shape
    fn = covariance.matern32
    x, ls, os_, Bt, v, d = make_inputs(9300, B, n, D, T, c)
    assert (_hip.load().lo_kernel_kron_mv_workspace_bytes(B, n, D, T, c) > 256) == (B == 1)
    assert torch.equal(direct(fn, x, ls, os_, Bt, v, d, "full"), direct(fn, x, ls, os_, Bt, v, d, "full"))


def test_error_codes_of_the_entry_point():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, T, c = 1, 300, 3, 2, 2
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    Bt = torch.eye(T, device=DEV).expand(B, T, T).contiguous()
    v = torch.randn(B, n * T, c, device=DEV)
    y = torch.full((B, n * T, c), -7.0, device=DEV)
    dfull = torch.ones(B, n * T, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_kron_mv_workspace_bytes(B, n, D, T, c)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(xx=x, th=theta, tk=Bt, fam=0, b=B, nn=n, dim=D, tt=T, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_kron_mv_f32(p(xx), p(th), p(tk), fam, b, nn, dim, tt, p(vv), cc, p(dd), mode, p(yy), p(w),
                                         wb, st)

    assert mv() == 0 and mv(dd=dfull, mode=1) == 0
    torch.cuda.synchronize()
    y.fill_(-7.0)
    for bad in (dict(xx=None), dict(th=None), dict(tk=None), dict(vv=None), dict(yy=None), dict(b=0), dict(nn=0),
                dict(nn=-1), dict(dim=0), dict(cc=0), dict(tt=0), dict(tt=-1), dict(fam=4), dict(fam=-1), dict(mode=1),
                dict(mode=2), dict(mode=3)):
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    wide, th33 = torch.rand(1, 10, 33, device=DEV), torch.ones(1, 34, device=DEV)
    v20, y20 = torch.randn(1, 20, 1, device=DEV), torch.full((1, 20, 1), -7.0, device=DEV)
    assert mv(xx=wide, th=th33, nn=10, dim=33, vv=v20, cc=1, yy=y20) == _hip.LO_ERR_UNSUPPORTED
    B9 = torch.eye(9, device=DEV).expand(1, 9, 9).contiguous()
    v90, y90 = torch.randn(1, 90, 1, device=DEV), torch.full((1, 90, 1), -7.0, device=DEV)
    assert mv(tk=B9, nn=10, tt=9, vv=v90, cc=1, yy=y90) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_kernel_kron_mv_workspace_bytes(1, 10, 33, 2, 1) == 0 and lib.lo_kernel_kron_mv_workspace_bytes(1, 10, 3, 9, 1) == 0
    # a short workspace is refused before anything is launched: y keeps its fill (as after every refusal above)
    assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((y20 == -7.0).all()) and bool((y90 == -7.0).all())


def test_error_codes_and_refusals_of_the_kind():
    """LO_OP_KERNEL_KRON_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; the float64
    entry points refuse the kind, a sum does not take it as a term and a mask not as its base."""
    lib, p = _hip.load(), _hip.ptr
    B, n, D, T, c = 1, 150, 3, 2, 2
    N = n * T
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    Bt = (torch.eye(T, device=DEV) + 0.2).expand(B, T, T).contiguous()
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_kron_diag_descriptor(x, theta, 3, Bt)
    assert desc.kind == _hip.LO_OP_KERNEL_KRON_DIAG and desc.n2 == 3 and desc.R == D and desc.N == N
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_kron_mv(x, theta, Bt, 3, v))
    y.fill_(-7.0)
    null = ctypes.cast(None, ctypes.POINTER(_hip.OpDesc))
    for field, val, rc in (("n2", 4, -1), ("n2", -1, -1), ("nterms", 0, -1), ("nterms", 7, -1), ("N", N + 1, -1),
                           ("A0", None, -1), ("A1", None, -1), ("terms", null, -1), ("R", 0, -1),
                           ("R", 33, _hip.LO_ERR_UNSUPPORTED)):
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, val)  # (nterms 7: N % T != 0)
    s = desc.c_struct()
    s.nterms, s.N = 10, 300  # (N % T == 0, T beyond LO_KERNEL_KRON_MAX_TASKS)
    assert run() == _hip.LO_ERR_UNSUPPORTED
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_kron_diag_descriptor(torch.rand(1, 10, 33, device=DEV), torch.ones(1, 34, device=DEV), 0, Bt) is None
    assert K.kernel_kron_diag_descriptor(x, theta, 0, torch.eye(9, device=DEV).expand(1, 9, 9)) is None
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
    for field, val, rc in (("n2", 4, -1), ("nterms", 0, -1), ("nterms", 7, -1), ("terms", null, -1),
                           ("R", 33, _hip.LO_ERR_UNSUPPORTED)):
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


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g40_kernel_kron_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in GRAD_NAMES:
            t[k].requires_grad_(True)
    return t


def kron_op(p, t, guard=True):
    fn = covariance.FAMILIES[CASES[p][0]]
    kern = KernelLinearOperator(t["x"], t["x"], guarded(fn, CASES[p][2]) if guard else fn, num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"])
    return KroneckerProductLinearOperator(kern, DenseLinearOperator(t["task"]))


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_kron {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(kron_op(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(Kron(Kernel, Bt) + Diag) under the reference run's solver settings, covar_func guarded against any dense
    evaluation: the descriptor kind (solve and inv_quad_logdet lower to it, not to LO_OP_CALLBACK: no closure reaches
    the solvers), the product, the diagonal, solve, inv_quad_logdet with injected probes, the pivoted Cholesky, backward."""
    G = golden(p)
    family, B, n, D, T, ard, seed = CASES[p]
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = kron_op(p, t)
        assert S._kernel_kron_refusal() is None
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_KRON_DIAG and desc.kernel_terms == T and desc.diag_mode == 1
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.A1.shape == (B, D + 1) and desc.N == n * T
        assert desc.task.data_ptr() == t["task"].data_ptr()
        const = AddedDiagLinearOperator(S, ConstantDiagLinearOperator(t["noise"][:, :1], n * T))._kernel_descriptor()
        assert const.kind == _hip.LO_OP_KERNEL_KRON_DIAG and const.diag_mode == 2
        check(G, p, "mv", S @ t["V"])
        check(G, p, "mv", K.kernel_kron_mv(desc.A0, desc.A1, desc.task, desc.n2, t["V"]))
        check(G, p, "diag", S.diagonal())
        # the solvers get the descriptor: a product through Python (the callback route of the parent) would run the
        # per-factor composition, whose kernel factor calls K.kernel_mv
        from linear_operator_amd.operators import kronecker_product_linear_operator as kp

        with mock.patch.object(kp, "_kron_matmul", side_effect=AssertionError("Python product")), \
                mock.patch.object(K, "kernel_mv", side_effect=AssertionError("Python product")), \
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
        Ag = AddedDiagLinearOperator(kron_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    check(G, p, "gl", tg["lengthscale"].grad)
    check(G, p, "go", tg["outputscale"].grad)
    check(G, p, "gx", tg["x"].grad)
    check(G, p, "gB", tg["task"].grad)


@pytest.mark.parametrize("p", list(CASES))
def test_gradients_through_inv_quad_against_fp64_autograd(p):
    """Lengthscale, outputscale, points and Bt through inv_quad of Kron(Kernel, Bt) + Diag on the matrix-free route,
    against float64 autograd on the dense matrix; the bound from the float32 run of the same computation (inv_quad under
    the same settings, autograd through the covariance function) on the STORED dense operator."""
    fn = covariance.FAMILIES[CASES[p][0]]
    x = inputs(p)

    def leaves(dtype):
        t = {k: dev(v, dtype) for k, v in x.items()}
        for k in GRAD_NAMES:
            t[k].requires_grad_(True)
        return t

    t64 = leaves(torch.float64)
    A64 = dense_kron(fn(t64["x"], t64["x"], t64["lengthscale"], t64["outputscale"]), t64["task"]) \
        + torch.diag_embed(t64["noise"])
    (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum().backward()
    with solver_settings(settings):
        ts = leaves(torch.float32)
        stored = dense_kron(fn(ts["x"], ts["x"], ts["lengthscale"], ts["outputscale"]), ts["task"])
        AddedDiagLinearOperator(DenseLinearOperator(stored), DiagLinearOperator(ts["noise"])).inv_quad(ts["rhs"]).sum().backward()
        tg = leaves(torch.float32)
        AddedDiagLinearOperator(kron_op(p, tg), DiagLinearOperator(tg["noise"])).inv_quad(tg["rhs"]).sum().backward()
    for k in GRAD_NAMES:
        want = host(t64[k].grad)
        within(f"inv_quad gradient {p} {k}", rel(host(tg[k].grad), want), rel(host(ts[k].grad), want))


def test_matmul_routing_follows_the_table():
    """`_matmul` of the product goes to lo_kernel_kron_mv_f32 exactly for the (T, columns) cells of the module's table;
    every other cell keeps the per-factor composition.  Both agree with the float64 composition either way."""
    from linear_operator_amd.operators import kronecker_product_linear_operator as kp

    fn = covariance.rbf
    for T in (2, 4):
        for c in (1, 5):
            B, n, D = 1, 130, 3
            x, ls, os_, Bt, v, d = make_inputs(9400 + T, B, n, D, T, c)
            Bt = 0.5 * (Bt + Bt.transpose(0, 2, 1))
            tx = dev(x)
            kern = KernelLinearOperator(tx, tx, guarded(fn, n), num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                                        outputscale=dev(os_))
            S = KroneckerProductLinearOperator(kern, DenseLinearOperator(dev(Bt)))
            assert S._kernel_kron_refusal() is None
            with mock.patch.object(K, "kernel_kron_mv", wraps=K.kernel_kron_mv) as fused, \
                    mock.patch.object(K, "kernel_mv", wraps=K.kernel_mv) as single:
                y = S._matmul(dev(v))
            routed = bool(kp._NATIVE_MATMUL_KERNEL_KRON.get((T, 1 if c == 1 else 2), False))
            assert (fused.call_count, single.call_count) == ((1, 0) if routed else (0, 1)), (T, c)
            want = host(composition(fn, x, ls, os_, Bt, v, d, "none", torch.float64))
            comp = host(composition(fn, x, ls, os_, Bt, v, d, "none", torch.float32))
            within(f"_matmul T={T} c={c} {'fused' if routed else 'composed'}", rel(host(y), want), rel(comp, want))


def test_product_never_holds_the_matrix():
    """n = 32768, T = 4, one column: the stored operator would be 64 GiB.  The allocator's peak grows by at most the
    sizer's bytes plus three copies of y, through the entry point and through the kind."""
    n, D, T, c = 32768, 4, 4, 1
    g = torch.Generator().manual_seed(9500)
    x = torch.rand(1, n, D, generator=g).to(DEV)
    ls, os_ = torch.full((1, 1, D), 0.3, device=DEV), torch.full((1,), 1.2, device=DEV)
    Bt = (torch.eye(T) + 0.2 * torch.rand(T, T, generator=g)).to(DEV)[None]
    v = torch.randn(1, n * T, c, generator=g).to(DEV)
    noise = (0.1 + torch.rand(1, n * T, generator=g)).to(DEV)
    theta = K.kernel_theta(ls, os_, (1,), D)
    allowed = _hip.load().lo_kernel_kron_mv_workspace_bytes(1, n, D, T, c) + 3 * v.numel() * 4
    kern = KernelLinearOperator(x, x, guarded(covariance.rbf, n), num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
    A = AddedDiagLinearOperator(KroneckerProductLinearOperator(kern, DenseLinearOperator(Bt)), DiagLinearOperator(noise))
    outs = []
    for label, call in (("entry", lambda: K.kernel_kron_mv(x, theta, Bt, 0, v, noise)), ("kind", lambda: A._matmul(v))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs.append(call())
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
        print(f"kernel_kron_mv n={n} T={T} {label}: peak growth {growth} bytes, allowed {allowed}")
        assert growth <= allowed, (label, growth, allowed)
    assert torch.equal(outs[0], outs[1])
    rows = covariance.rbf(x[0, :2].double(), x[0].double(), ls[0].double(), os_[0].double())  # [2, n]
    w = torch.einsum("ts,jsc->jtc", Bt[0].double(), v[0].double().reshape(n, T, c))
    want = torch.einsum("ij,jtc->itc", rows, w).reshape(2 * T, c) + noise[0, : 2 * T, None].double() * v[0, : 2 * T].double()
    assert rel(host(outs[0][0, : 2 * T]), host(want)) <= 1e-5
