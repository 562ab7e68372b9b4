"""KernelLinearOperator on the MI355X: lo_kernel_mv_f32 / lo_kernel_bilinear_f32 (csrc/lo_kernel_op.hip) against fp64
numpy, the kind LO_OP_KERNEL_DIAG through the public API (solve, inv_quad_logdet, roots, sqrt_inv_matmul, gradients) and
the pivoted Cholesky against the reference's goldens (tests/golden/g38_kernel_op_*.npz).

Bounds.  Golden quantities: the error against the fixture's float64 value is at most REF_FACTOR = 4 times the reference's
own recorded float32 error (floored at 1e-7).  Products without a golden: 4 times the error of the torch float32 dense
composition `covariance.f(x1, x2, ..) @ v` measured on the same inputs inside the test (same floor).  Every test prints
the ratio it measured (DESIGN.md section 6l holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_op import CASES, ERR_FLOOR, PROBES, RANK, inputs, rel, solver_settings  # noqa: E402
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, KernelLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
FAMILY_NAMES = ["rbf", "matern12", "matern32", "matern52"]
REF_ORDERS = 8  # orderings of the points over which the float32 reference's error of a gradient is measured


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().double().cpu().numpy()


def g64(name, r):
    return {"rbf": np.exp(-r ** 2 / 2), "matern12": np.exp(-r),
            "matern32": (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r),
            "matern52": (1 + np.sqrt(5) * r + 5 * r ** 2 / 3) * np.exp(-np.sqrt(5) * r)}[name]


def dense64(name, x1, x2, ls, os_):
    """K [B, M, N] in float64 numpy from the float32 inputs."""
    x1, x2, ls, os_ = (np.asarray(a, dtype=np.float64) for a in (x1, x2, ls, os_))
    a, b = x1 / ls, x2 / ls
    r2 = np.zeros((x1.shape[0], x1.shape[1], x2.shape[1]))
    for k in range(x1.shape[-1]):  # (one dimension at a time: no [B, M, N, D] temporary)
        r2 += (a[:, :, None, k] - b[:, None, :, k]) ** 2
    return os_[:, None, None] ** 2 * g64(name, np.sqrt(r2))


def make_points(seed, B, M, N, D, ard, kind="plain"):
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
    ls = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    os_ = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    return x1, x2, ls, os_


def theta_of(ls, os_, D):
    return K.kernel_theta(dev(ls), dev(os_), (ls.shape[0],), D)


# (family, B, M, N, D, c, ARD, diagonal): every family meets every D; every N, c, B, rectangular pair, lengthscale form and
# diagonal mode appears
PRODUCT_CASES = [
    ("rbf", 1, 1, 1, 1, 1, False, "none"), ("rbf", 3, 63, 63, 3, 4, True, "full"),
    ("rbf", 1, 257, 257, 8, 17, False, "const"), ("rbf", 1, 1013, 1013, 32, 33, True, "none"),
    ("matern12", 1, 63, 63, 1, 4, True, "const"), ("matern12", 1, 257, 257, 3, 17, False, "none"),
    ("matern12", 3, 1013, 1013, 8, 1, True, "full"), ("matern12", 1, 1, 1, 32, 33, False, "full"),
    ("matern32", 1, 257, 257, 1, 33, False, "full"), ("matern32", 1, 1013, 1013, 3, 1, True, "const"),
    ("matern32", 3, 1, 1, 8, 4, False, "none"), ("matern32", 1, 63, 63, 32, 17, True, "none"),
    ("matern52", 3, 1013, 1013, 1, 17, True, "none"), ("matern52", 1, 1, 1, 3, 33, False, "const"),
    ("matern52", 1, 63, 63, 8, 1, True, "full"), ("matern52", 1, 257, 257, 32, 4, False, "full"),
    ("rbf", 3, 130, 77, 3, 4, True, "none"), ("matern52", 1, 77, 130, 8, 17, False, "none"),
    ("matern32", 1, 130, 77, 32, 1, True, "none"), ("matern12", 3, 77, 130, 1, 33, False, "none"),
]


def product_check(name, x1, x2, ls, os_, v, d, diag, label):
    """lo_kernel_mv_f32 and the operator's _matmul against fp64 numpy; the bound from the torch float32 composition."""
    B, M, D = x1.shape
    N = x2.shape[1]
    fn = covariance.FAMILIES[name]
    want = dense64(name, x1, x2, ls, os_) @ v.astype(np.float64)
    dd = None
    if diag == "full":
        dd = d
        want = want + d[:, :, None].astype(np.float64) * v
    elif diag == "const":
        dd = d[:, 0]
        want = want + d[:, :1, None].astype(np.float64) * v
    tx1, tx2, tls, tos, tv = dev(x1), dev(x2), dev(ls), dev(os_), dev(v)
    comp = fn(tx1, tx2, tls, tos) @ tv
    if dd is not None:
        comp = comp + (dev(dd)[:, :, None] if diag == "full" else dev(dd)[:, None, None]) * tv
    ref_err = max(rel(host(comp), want), ERR_FLOOR)
    y = K.kernel_mv(tx1, tx2, theta_of(ls, os_, D), fn.native_family, tv, None if dd is None else dev(dd),
                    const_diag=diag == "const")
    assert torch.isfinite(y).all()
    err = rel(host(y), want)
    print(f"kernel_mv {label}: err {err:.3e} torch fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)
    # the operator: the same kernel through _matmul (rectangular) or through the kind LO_OP_KERNEL_DIAG (square + diagonal)
    op = KernelLinearOperator(tx1, tx1 if x2 is x1 else tx2, fn, num_nonbatch_dimensions=NB, lengthscale=tls,
                              outputscale=tos)
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        if dd is None:
            assert torch.equal(op._matmul(tv), y)
            assert (op._kernel_descriptor() is not None) == (x2 is x1)
        else:
            diag_op = DiagLinearOperator(dev(dd)) if diag == "full" else ConstantDiagLinearOperator(dev(dd)[:, None], N)
            A = AddedDiagLinearOperator(op, diag_op)
            desc = A._kernel_descriptor()
            assert desc.kind == _hip.LO_OP_KERNEL_DIAG and desc.diag_mode == (1 if diag == "full" else 2)
            assert torch.equal(A._matmul(tv), y)
    return y


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_product_against_fp64_numpy(case):
    name, B, M, N, D, c, ard, diag = case
    seed = 6000 + 7 * PRODUCT_CASES.index(case)
    x1, x2, ls, os_ = make_points(seed, B, M, N, D, ard)
    g = rng(seed + 1)
    v = g.standard_normal((B, N, c)).astype(np.float32)
    d = (0.05 + g.random((B, N))).astype(np.float32)
    product_check(name, x1, x2, ls, os_, v, d, diag, "-".join(str(x) for x in case))


@pytest.mark.parametrize("name", FAMILY_NAMES)
@pytest.mark.parametrize("kind", ["dup", "far"])
def test_product_with_coincident_and_with_far_points(name, kind):
    B, N, D, c = 1, 257, 3, 4
    x1, x2, ls, os_ = make_points(6300, B, N, N, D, True, kind)
    v = rng(6301).standard_normal((B, N, c)).astype(np.float32)
    y = product_check(name, x1, x2, ls, os_, v, None, "none", f"{name}-{kind}")
    if kind == "far":  # only the diagonal survives: y = os^2 v
        assert rel(host(y), os_[:, None, None].astype(np.float64) ** 2 * v) <= 1e-6


def test_product_without_a_column_split():
    """B ceil(M / 256) >= 512 workgroups: one workgroup sweeps all the tiles of its rows (no partials, no second pass)."""
    B, M, N, D, c = 128, 1024, 300, 1, 1
    g = torch.Generator().manual_seed(6400)
    x1, x2 = torch.rand(B, M, D, generator=g).to(DEV), torch.rand(B, N, D, generator=g).to(DEV)
    ls = (0.2 + 0.3 * torch.rand(B, 1, D, generator=g)).to(DEV)
    os_ = (0.8 + torch.rand(B, generator=g)).to(DEV)
    v = torch.randn(B, N, c, generator=g).to(DEV)
    assert _hip.load().lo_kernel_mv_workspace_bytes(B, M, N, D, c) == 256  # (nothing but the tail: no partials)
    want = host(covariance.matern32(x1.double(), x2.double(), ls.double(), os_.double()) @ v.double())
    ref_err = max(rel(host(covariance.matern32(x1, x2, ls, os_) @ v), want), ERR_FLOOR)
    y = K.kernel_mv(x1, x2, K.kernel_theta(ls, os_, (B,), D), covariance.matern32.native_family, v)
    err = rel(host(y), want)
    print(f"kernel_mv no-split: err {err:.3e} torch fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err


def _mv_args(B=1, M=300, N=300, D=3, c=2):
    x = torch.rand(B, M, D, device=DEV)
    x2 = x if M == N else torch.rand(B, N, D, device=DEV)
    theta = torch.ones(B, D + 1, device=DEV)
    v = torch.randn(B, N, c, device=DEV)
    y = torch.full((B, M, c), -7.0, device=DEV)
    return x, x2, theta, v, y


def test_error_codes_of_the_entry_points():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, c = 1, 300, 300, 3, 2
    x, x2, theta, v, y = _mv_args(B, M, N, D, c)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_mv_workspace_bytes(B, M, N, D, c)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(x1=x, xb=x2, th=theta, fam=0, b=B, m=M, n=N, dim=D, vv=v, cc=c, yy=y, w=ws, wb=need):
        return lib.lo_kernel_mv_f32(p(x1), p(xb), p(th), fam, b, m, n, dim, p(vv), cc, None, 0, p(yy), p(w), wb, st)

    assert mv() == 0
    for bad in (dict(x1=None), dict(xb=None), dict(th=None), dict(vv=None), dict(yy=None), dict(b=0), dict(m=0),
                dict(n=-1), dict(dim=0), dict(cc=0), dict(fam=4), dict(fam=-1)):
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG
    assert lib.lo_kernel_mv_f32(p(x), p(x2), p(theta), 0, B, M, N, D, p(v), c, None, 1, p(y), p(ws), need, st) == -1
    wide = torch.rand(1, 10, 33, device=DEV)
    th33, v10, y10 = torch.ones(1, 34, device=DEV), torch.randn(1, 10, 1, device=DEV), torch.empty(1, 10, 1, device=DEV)
    assert lib.lo_kernel_mv_f32(p(wide), p(wide), p(th33), 0, 1, 10, 10, 33, p(v10), 1, None, 0, p(y10), p(ws), need,
                                st) == _hip.LO_ERR_UNSUPPORTED
    # a short workspace is refused before anything is launched: y keeps its fill
    y.fill_(-7.0)
    assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    # the derivative
    U, g = torch.randn(B, M, 2, device=DEV), torch.full((B, D + 1), -7.0, device=DEV)
    gneed = lib.lo_kernel_bilinear_workspace_bytes(B, M, N, D, 2)
    gws = torch.empty(gneed, dtype=torch.uint8, device=DEV)

    def bil(x1=x, th=theta, fam=0, dim=D, uu=U, t=2, gg=g, w=gws, wb=gneed):
        return lib.lo_kernel_bilinear_f32(p(x1), p(x2), p(th), fam, B, M, N, dim, p(uu), p(v), t, p(gg), p(w), wb, st)

    assert bil() == 0
    for bad in (dict(x1=None), dict(th=None), dict(uu=None), dict(gg=None), dict(t=0), dict(fam=7), dict(dim=0)):
        assert bil(**bad) == -1, bad
    assert bil(dim=33) == _hip.LO_ERR_UNSUPPORTED
    g.fill_(-7.0)
    assert bil(wb=gneed - 1) == -3
    torch.cuda.synchronize()
    assert bool((g == -7.0).all())
    # the kind through lo_matvec_f32: D beyond the limit, an unknown family
    desc = K.kernel_diag_descriptor(x, theta, 0)
    s = desc.c_struct()
    s.n2 = 9
    assert lib.lo_matvec_workspace_bytes(ctypes.byref(s), c) >= 256
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st) == -1
    assert K.kernel_diag_descriptor(wide, th33, 0) is None


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_two_calls_give_the_same_bits(name):
    B, M, N, D, c = 3, 1013, 700, 8, 5
    x1, x2, ls, os_ = make_points(6500, B, M, N, D, True)
    fam = covariance.FAMILIES[name].native_family
    th = theta_of(ls, os_, D)
    v, U = torch.randn(B, N, c, device=DEV), torch.randn(B, M, c, device=DEV)
    assert torch.equal(K.kernel_mv(dev(x1), dev(x2), th, fam, v), K.kernel_mv(dev(x1), dev(x2), th, fam, v))
    assert torch.equal(K.kernel_bilinear(dev(x1), dev(x2), th, fam, U, v), K.kernel_bilinear(dev(x1), dev(x2), th, fam, U, v))


BILINEAR_CASES = [("rbf", 1, 257, 257, 3, 1, True, "plain"), ("matern12", 3, 130, 77, 1, 9, False, "plain"),
                  ("matern32", 1, 77, 130, 8, 4, True, "plain"), ("matern52", 1, 63, 63, 32, 2, False, "plain"),
                  ("rbf", 1, 64, 64, 2, 3, True, "dup"), ("matern12", 1, 64, 64, 2, 3, True, "dup"),
                  ("matern32", 1, 64, 64, 2, 3, False, "dup"), ("matern52", 1, 64, 64, 2, 3, True, "dup")]


@pytest.mark.parametrize("case", BILINEAR_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_hyperparameter_derivative_against_fp64_autograd(case):
    """lo_kernel_bilinear_f32 behind _bilinear_derivative: lengthscale and outputscale gradients of sum_s u_s^T K v_s
    against float64 autograd of the covariance function; the bound from float32 autograd of the same function (the
    root mean square of its error over REF_ORDERS orderings of the points, see below)."""
    name, B, M, N, D, t, ard, kind = case
    fn = covariance.FAMILIES[name]
    x1, x2, ls, os_ = make_points(6600 + BILINEAR_CASES.index(case), B, M, N, D, ard, kind)
    g = rng(6650)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)

    def autograd(dtype, pm=None, pn=None):
        """Gradients through the dense covariance function, the points (and the rows of U, V) taken in the order pm, pn:
        the same sums, rounded along another path."""
        pm = np.arange(M) if pm is None else pm
        pn = np.arange(N) if pn is None else pn
        tl, to = dev(ls).to(dtype).requires_grad_(True), dev(os_).to(dtype).requires_grad_(True)
        a, b = dev(x1[:, pm]).to(dtype), dev(x2[:, pn]).to(dtype)
        (dev(U[:, pm]).to(dtype) * (fn(a, b, tl, to) @ dev(V[:, pn]).to(dtype))).sum().backward()
        return host(tl.grad), host(to.grad)

    gl64, go64 = autograd(torch.float64)
    # The float32 reference's error is measured over REF_ORDERS orderings of the points and taken as their root mean
    # square: the outputscale gradient is ONE number per member, and the error of a single float32 evaluation of one
    # number is a draw that can land near zero -- a bound of 4 such draws would test luck, not accuracy.
    ref32 = []
    for k in range(REF_ORDERS):
        pm = rng(6660 + k).permutation(M)
        pn = pm if x2 is x1 else rng(6680 + k).permutation(N)
        ref32.append(autograd(torch.float32, pm, pn))
    rms = lambda want, idx: float(np.sqrt(np.mean([rel(r[idx], want) ** 2 for r in ref32])))  # noqa: E731
    gl_ref, go_ref = rms(gl64, 0), rms(go64, 1)
    tl, to = dev(ls).requires_grad_(True), dev(os_).requires_grad_(True)
    a = dev(x1)
    op = KernelLinearOperator(a, a if x2 is x1 else dev(x2), fn, num_nonbatch_dimensions=NB, lengthscale=tl, outputscale=to)
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        gx1, gx2, gl, go = op._bilinear_derivative(dev(U), dev(V))
    assert gx1 is None and gx2 is None and gl.shape == tl.shape and go.shape == to.shape
    assert torch.isfinite(gl).all() and torch.isfinite(go).all()
    for label, got, want, ref in (("lengthscale", gl, gl64, gl_ref), ("outputscale", go, go64, go_ref)):
        err, ref_err = rel(host(got), want), max(ref, ERR_FLOOR)
        print(f"kernel_bilinear {'-'.join(str(x) for x in case)} {label}: err {err:.3e} torch fp32 {ref_err:.3e} "
              f"ratio {err / ref_err:.2f}")
        assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def test_product_never_holds_the_matrix():
    """N = 32768: a dense K would be 4 GiB; the product may allocate 64 N (D + c) floats."""
    N, D, c = 32768, 4, 1
    g = torch.Generator().manual_seed(6700)
    x = torch.rand(N, D, generator=g).to(DEV)
    ls, os_ = torch.full((1, D), 0.3, device=DEV), torch.tensor(1.2, device=DEV)
    v = torch.randn(N, c, generator=g).to(DEV)
    op = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        y = op._matmul(v)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"kernel_mv N={N}: peak growth {growth} bytes, allowed {64 * N * (D + c) * 4}")
    assert growth < 64 * N * (D + c) * 4
    rows = covariance.rbf(x[:8].double(), x.double(), ls.double(), os_.double()) @ v.double()
    assert rel(host(y[:8]), host(rows)) <= 1e-5


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g38_kernel_op_{p}.npz"))


def tensors(p, grad=False):
    t = {k: dev(v) for k, v in inputs(p).items()}
    if grad:
        for k in ("x", "lengthscale", "outputscale"):
            t[k].requires_grad_(True)
    return t


def kernel_op(p, t):
    return KernelLinearOperator(t["x"], t["x"], covariance.FAMILIES[CASES[p][0]], num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"])


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_op {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def no_dense():
    return mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation"))


@pytest.mark.parametrize("p", list(CASES))
def test_product_diagonal_and_entries_against_the_goldens(p):
    G, t = golden(p), tensors(p)
    op = kernel_op(p, t)
    with no_dense():
        check(G, p, "mv", op @ t["V"])
        check(G, p, "diag", op.diagonal())
        check(G, p, "idx", op[t["ib"], t["ir"], t["ic"]])
        rows = op._get_rows(torch.zeros(op.batch_shape, dtype=torch.long, device=DEV) + 2)
    assert rel(host(rows), host(op.to_dense()[..., 2, :])) <= 1e-6


@pytest.mark.parametrize("p", list(CASES))
def test_pivoted_cholesky_against_the_goldens(p):
    G, t = golden(p), tensors(p)
    op = kernel_op(p, t)
    with no_dense():
        L, piv = op.pivoted_cholesky(RANK, return_pivots=True)
        L2, piv2 = op.pivoted_cholesky(RANK, return_pivots=True)
    assert np.array_equal(piv[..., :RANK].cpu().numpy(), G["piv"])
    check(G, p, "L", L)
    assert torch.equal(L, L2) and torch.equal(piv, piv2)


def test_pivoted_cholesky_entry_point_refuses_what_the_kind_does_not_take():
    lib, t = _hip.load(), tensors("m12")
    desc = kernel_op("m12", t)._kernel_descriptor()
    s = desc.c_struct()
    need = lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(s), 5)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    L, perm = torch.empty(1, 5, 63, device=DEV), torch.empty(1, 63, dtype=torch.int64, device=DEV)
    rank = ctypes.c_int32(0)
    st = _hip.stream_ptr(L.device)
    args = (5, 1e-3, _hip.ptr(L), _hip.ptr(perm), ctypes.byref(rank), _hip.ptr(ws), need, st)
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == 0 and rank.value == 5
    s.n2 = 4
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == -1
    s.n2, s.R = 0, 33
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == _hip.LO_ERR_UNSUPPORTED
    s.R = 1
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, _hip.ptr(L), _hip.ptr(perm), ctypes.byref(rank),
                                       _hip.ptr(ws), need, st) == _hip.LO_ERR_UNSUPPORTED


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(kernel_op(p, t), DiagLinearOperator(t["noise"]))


def test_public_api_end_to_end_at_n_1013():
    """AddedDiag(Kernel, Diag) at N = 1013 with the rank-15 preconditioner forced: solve, inv_quad_logdet, the Lanczos
    root, sqrt_inv_matmul and the gradients of inv_quad, all on the native route (the dense evaluation is a spy)."""
    p = "m52"
    G = golden(p)
    with solver_settings(settings), settings.num_trace_samples(PROBES), no_dense():
        t = tensors(p)
        A = AddedDiagLinearOperator(kernel_op(p, t), DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc.kind == _hip.LO_OP_KERNEL_DIAG and desc.N == 1013 and desc.R == 8 and desc.n2 == 3
        check(G, p, "solve", A.solve(t["rhs"]))
        iq, ld = probed(p, t).inv_quad_logdet(t["rhs"], logdet=True)
        check(G, p, "iq", iq)
        check(G, p, "ld", ld)
        check(G, p, "sqrt", A.sqrt_inv_matmul(t["rhs"]))
        R = A.root_decomposition().root.to_dense()
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(kernel_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    x64 = {k: torch.from_numpy(v).double().to(DEV) for k, v in inputs(p).items() if v.dtype.kind == "f"}
    K64 = covariance.matern52(x64["x"], x64["x"], x64["lengthscale"], x64["outputscale"]) + torch.diag_embed(x64["noise"])
    err, ref_err = rel(host(R.double() @ R.double().mT), host(K64)), float(G["root_err"])
    print(f"kernel_op {p} root: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err
    check(G, p, "gl", tg["lengthscale"].grad)
    check(G, p, "go", tg["outputscale"].grad)
    check(G, p, "gx", tg["x"].grad)


@pytest.mark.parametrize("p", ["rbf", "m12", "m32"])
def test_solve_and_gradients_at_the_smaller_goldens(p):
    G = golden(p)
    with solver_settings(settings), no_dense():
        t = tensors(p)
        A = AddedDiagLinearOperator(kernel_op(p, t), DiagLinearOperator(t["noise"]))
        assert A._kernel_descriptor().kind == _hip.LO_OP_KERNEL_DIAG
        check(G, p, "solve", A.solve(t["rhs"]))
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(kernel_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    check(G, p, "gl", tg["lengthscale"].grad)
    check(G, p, "go", tg["outputscale"].grad)
    check(G, p, "gx", tg["x"].grad)


def test_outside_the_gate_the_general_path_serves_on_the_device():
    g = torch.Generator().manual_seed(6800)
    x = torch.rand(40, 33, generator=g).to(DEV)
    v = torch.randn(40, 2, generator=g).to(DEV)
    ls, os_ = torch.full((1, 1), 2.0, device=DEV), torch.tensor(1.1, device=DEV)
    wide = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
    assert wide._kernel_descriptor() is None and not wide._is_native()
    assert torch.allclose(wide._matmul(v), covariance.rbf(x, x, ls, os_) @ v)
    x64 = x[:, :3].double()
    dbl = KernelLinearOperator(x64, x64, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=ls.double(),
                               outputscale=os_.double())
    assert dbl._kernel_descriptor() is None
    assert torch.allclose(dbl._matmul(v.double()), covariance.rbf(x64, x64, ls.double(), os_.double()) @ v.double())
