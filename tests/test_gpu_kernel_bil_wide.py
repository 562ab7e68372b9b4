"""The many-column derivatives of the matrix-free kernel operator on the MI355X: lo_kernel_bilinear_wide_f32 and
lo_kernel_points_grad_wide_f32 (csrc/lo_kernel_bil_wide.hip, W = U V^T on v_mfma_f32_32x32x2_f32, rows handed back to one
lane each by v_permlane32_swap_b32) against float64 autograd of the covariance functions.  The bounds are those of
test_hyperparameter_derivative_against_fp64_autograd (REF_FACTOR times the root mean square error of float32 autograd
over REF_ORDERS orderings of the points) and of tests/test_gpu_kernel_points_grad.py (REF_FACTOR times the float32 autograd
error), both floored at ERR_FLOOR; every case prints its ratio (DESIGN.md section 6y holds the table)."""
import numpy as np
import pytest
import torch

from test_gpu_kernel_op import (DEV, ERR_FLOOR, NB, REF_FACTOR, REF_ORDERS, dev, host, make_points, no_dense, rel, rng,
                                theta_of)

from linear_operator_amd import _hip, covariance
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import KernelLinearOperator

pytestmark = pytest.mark.gpu

# (family, B, M, N, D, t, ARD, points).  M: the 32-row tile and the half-wave swap (31, 33), a second wave (65), a second
# workgroup (257); N: the 32-point MFMA block (31, 33), the LDS tile with js > 1 (127, 129, 257); t: an odd last contraction
# step (1, 3, 9, 17), a full sweep (32), a second one (33, 65); every family meets every padded D.  M = N = 1 is left out:
# with one coincident pair both derivatives are exactly 0 and a relative error has no meaning.
FAMS = ["rbf", "matern12", "matern32", "matern52"]
CASES = [
    ("rbf", 1, 1, 2, 1, 1, False, "plain"), ("rbf", 3, 31, 127, 3, 2, True, "plain"),
    ("rbf", 1, 257, 257, 8, 17, False, "plain"), ("rbf", 1, 65, 129, 16, 32, True, "plain"),
    ("rbf", 1, 33, 3, 32, 33, False, "plain"),
    ("matern12", 1, 65, 129, 1, 65, True, "plain"), ("matern12", 1, 257, 2, 3, 3, False, "plain"),
    ("matern12", 3, 33, 257, 8, 9, True, "plain"), ("matern12", 1, 1, 127, 16, 17, False, "plain"),
    ("matern12", 1, 31, 31, 32, 8, True, "plain"),
    ("matern32", 1, 65, 1, 1, 33, True, "plain"), ("matern32", 1, 33, 33, 3, 65, False, "plain"),
    ("matern32", 1, 31, 129, 8, 1, True, "plain"), ("matern32", 3, 257, 257, 16, 2, False, "plain"),
    ("matern32", 1, 33, 2, 32, 17, True, "plain"),
    ("matern52", 1, 257, 127, 1, 32, False, "plain"), ("matern52", 1, 33, 31, 3, 33, True, "plain"),
    ("matern52", 1, 65, 257, 8, 65, False, "plain"), ("matern52", 3, 31, 3, 16, 3, True, "plain"),
    ("matern52", 1, 257, 257, 32, 9, False, "plain"),
    ("rbf", 3, 130, 77, 3, 17, True, "plain"), ("matern52", 1, 77, 130, 8, 33, False, "plain"),
    ("matern32", 512, 33, 129, 3, 17, True, "plain"),  # B ceil(M / 256) = 512: no column split
] + [(f, 1, 257, 257, 3, 17, True, kind) for f in FAMS for kind in ("dup", "far")]
IDS = ["-".join(str(x) for x in c) for c in CASES]


def inputs(case):
    name, B, M, N, D, t, ard, kind = case
    seed = 8000 + 7 * CASES.index(case)
    x1, x2, ls, os_ = make_points(seed, B, M, N, D, ard, kind)
    g = rng(seed + 1)
    U, V = g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)
    return covariance.FAMILIES[name], x1, x2, ls, os_, U, V


def autograd(fn, x1, x2, ls, os_, U, V, dtype, pm=slice(None), pn=slice(None)):
    """(d / d x1 with x2 held fixed, d / d lengthscale, d / d outputscale) of sum(U * (K @ V)) through the dense covariance
    function in `dtype`, the points and the rows of U, V taken in the order pm, pn."""
    a, tl, to = (dev(z).to(dtype).requires_grad_(True) for z in (x1[:, pm], ls, os_))
    (dev(U[:, pm]).to(dtype) * (fn(a, dev(x2[:, pn]).to(dtype), tl, to) @ dev(V[:, pn]).to(dtype))).sum().backward()
    return host(a.grad), host(tl.grad), host(to.grad)


def within(label, got, want, ref_err):
    err, ref_err = rel(host(got), want), max(ref_err, ERR_FLOOR)
    print(f"{label}: err {err:.3e} torch fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert torch.isfinite(got).all() and err <= REF_FACTOR * ref_err, (label, err, ref_err)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_hyperparameter_derivative_against_fp64_autograd(case):
    name, B, M, N, D, t, ard, kind = case
    fn, x1, x2, ls, os_, U, V = inputs(case)
    _, gl64, go64 = autograd(fn, x1, x2, ls, os_, U, V, torch.float64)
    ref32 = []
    for k in range(REF_ORDERS):
        pm = rng(8500 + k).permutation(M)
        ref32.append(autograd(fn, x1, x2, ls, os_, U, V, torch.float32, pm, pm if x2 is x1 else rng(8600 + k).permutation(N)))
    rms = lambda want, idx: float(np.sqrt(np.mean([rel(r[idx], want) ** 2 for r in ref32])))  # noqa: E731
    theta = theta_of(ls, os_, D)
    args = (dev(x1), dev(x2), theta, fn.native_family, dev(U), dev(V))
    gt = K.kernel_bilinear_wide(*args)
    assert torch.equal(K.kernel_bilinear_wide(*args), gt)  # two calls give equal bits
    d_ls = (-(theta[:, :D] ** 2) * gt[:, :D]).reshape(B, 1, D)  # (the chain rule of KernelLinearOperator._theta_to_params)
    d_ls = d_ls if ard or D == 1 else d_ls.sum(-1, keepdim=True)
    assert torch.isfinite(gt).all()
    if kind != "far":  # (far points: every off-diagonal pair underflows and the lengthscale derivative is 0)
        within(f"kernel_bilinear_wide {IDS[CASES.index(case)]} lengthscale", d_ls, gl64, rms(gl64, 1))
    within(f"kernel_bilinear_wide {IDS[CASES.index(case)]} outputscale", 2.0 * dev(os_) * gt[:, D], go64, rms(go64, 2))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_points_gradient_against_fp64_autograd(case):
    name, B, M, N, D, t, ard, kind = case
    fn, x1, x2, ls, os_, U, V = inputs(case)
    want = autograd(fn, x1, x2, ls, os_, U, V, torch.float64)[0]
    ref = autograd(fn, x1, x2, ls, os_, U, V, torch.float32)[0]
    if B == 512:
        assert _hip.load().lo_kernel_points_grad_wide_workspace_bytes(B, M, N, D, t) == 256  # (nothing but the tail)
    args = (dev(x1), dev(x2), theta_of(ls, os_, D), fn.native_family, dev(U), dev(V))
    g = K.kernel_points_grad_wide(*args)
    assert g.shape == (B, M, D) and torch.equal(K.kernel_points_grad_wide(*args), g)  # two calls give equal bits
    if kind == "far":
        assert np.abs(want).max() <= 1e-12 and bool((g == 0).all())
    else:
        within(f"kernel_points_grad_wide {IDS[CASES.index(case)]}", g, want, rel(ref, want))


def test_wide_entry_points_return_the_error_codes_of_their_plain_twins():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, t = 1, 300, 300, 3, 17
    x, theta = torch.rand(B, M, D, device=DEV), torch.ones(B, D + 1, device=DEV)
    U, V = torch.randn(B, M, t, device=DEV), torch.randn(B, N, t, device=DEV)
    st = _hip.stream_ptr(x.device)
    for stem, shape in (("lo_kernel_bilinear", (B, D + 1)), ("lo_kernel_points_grad", (B, M, D))):
        g = torch.full(shape, -7.0, device=DEV)
        need = getattr(lib, stem + "_wide_workspace_bytes")(B, M, N, D, t)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)

        def both(x1=x, dim=D, w=ws, wb=need):
            a = (p(x1), p(x), p(theta), 0, B, M, N, dim, p(U), p(V), t, p(g), p(w), wb, st)
            codes = getattr(lib, stem + "_wide_f32")(*a), getattr(lib, stem + "_f32")(*a)
            assert codes[0] == codes[1], (stem, codes)
            return codes[0]

        assert both(x1=None) == -1 and both(dim=33) == _hip.LO_ERR_UNSUPPORTED
        assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: g keeps its fill
        torch.cuda.synchronize()
        assert bool((g == -7.0).all()) and both() == 0


def test_the_operator_takes_the_wide_kernels_where_the_rule_says_so():
    """The route through kernel_bil_run / kernel_pgrad_run (one gate: ko_bil_wide of csrc/lo_kernel_shape.h): t = 17 goes to
    the wide kernels, t = 4 keeps the plain entry points' own."""
    D, fn = 3, covariance.matern52
    x1, _, ls, os_ = make_points(8700, 3, 300, 300, D, True)
    theta = theta_of(ls, os_, D)
    for t, bil, pg in ((17, K.kernel_bilinear_wide, K.kernel_points_grad_wide), (4, K.kernel_bilinear, K.kernel_points_grad)):
        U, V = torch.randn(3, 300, t, device=DEV), torch.randn(3, 300, t, device=DEV)
        tx, tl, to = (dev(z).requires_grad_(True) for z in (x1, ls, os_))
        op = KernelLinearOperator(tx, tx, fn, num_nonbatch_dimensions=NB, lengthscale=tl, outputscale=to)
        with no_dense():
            gx1, gx2, gl, go = op._bilinear_derivative(U, V)
        args = (tx.detach(), tx.detach(), theta, fn.native_family)
        gt = bil(*args, U, V)
        assert torch.equal(gx1, pg(*args, U, V)) and torch.equal(gx2, pg(*args, V, U))
        assert torch.equal(gl, (-(theta[:, :D] ** 2) * gt[:, :D]).reshape(3, 1, D))
        assert torch.equal(go, 2.0 * to.detach() * gt[:, D])
