"""The many-column product of the matrix-free kernel operator on the MI355X: lo_kernel_mv_wide_f32
(csrc/lo_kernel_mv_wide.hip, kernel values on the vector ALU, their product with V on v_mfma_f32_32x32x2_f32) against
fp64 numpy.  The bound is the one of tests/test_gpu_kernel_op.py: at most REF_FACTOR = 4 times the error of the torch
float32 composition `covariance.f(x1, x2, ..) @ v` on the same inputs, floored at ERR_FLOOR; every case prints its ratio."""
import numpy as np
import pytest
import torch

from test_gpu_kernel_op import (DEV, ERR_FLOOR, NB, REF_FACTOR, dense64, dev, golden, host, kernel_op, make_points,
                                no_dense, rel, rng, solver_settings, tensors, theta_of)

from linear_operator_amd import _hip, covariance, settings
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

pytestmark = pytest.mark.gpu

# (family, B, M, N, D, c, ARD, diagonal, points).  M: a 32-row tile, a wave's two tiles, the workgroup edge; N: an odd last
# MFMA step, the 128-point tile edge, js > 1 (N > 128); c: a ragged last sweep of 32; every family meets every D.
FAMS = ["rbf", "matern12", "matern32", "matern52"]
CASES = [
    ("rbf", 1, 1, 1, 1, 1, False, "full", "plain"), ("rbf", 3, 31, 127, 3, 5, True, "none", "plain"),
    ("rbf", 1, 257, 257, 8, 17, False, "const", "plain"), ("rbf", 1, 65, 129, 16, 32, True, "none", "plain"),
    ("rbf", 1, 33, 3, 32, 33, False, "none", "plain"),
    ("matern12", 1, 129, 129, 1, 65, True, "full", "plain"), ("matern12", 1, 257, 2, 3, 1, False, "none", "plain"),
    ("matern12", 3, 33, 257, 8, 5, True, "none", "plain"), ("matern12", 1, 1, 127, 16, 17, False, "none", "plain"),
    ("matern12", 1, 127, 127, 32, 32, True, "const", "plain"),
    ("matern32", 1, 65, 1, 1, 33, True, "none", "plain"), ("matern32", 1, 3, 3, 3, 65, False, "const", "plain"),
    ("matern32", 1, 31, 129, 8, 1, True, "none", "plain"), ("matern32", 3, 257, 257, 16, 5, False, "full", "plain"),
    ("matern32", 1, 33, 2, 32, 17, True, "none", "plain"),
    ("matern52", 1, 257, 127, 1, 32, False, "none", "plain"), ("matern52", 1, 2, 2, 3, 33, True, "full", "plain"),
    ("matern52", 1, 65, 257, 8, 65, False, "none", "plain"), ("matern52", 3, 31, 3, 16, 1, True, "none", "plain"),
    ("matern52", 1, 257, 257, 32, 5, False, "const", "plain"),
    ("rbf", 3, 130, 77, 3, 17, True, "none", "plain"), ("matern52", 1, 77, 130, 8, 33, False, "none", "plain"),
    ("matern32", 512, 33, 129, 3, 17, True, "none", "plain"),  # B ceil(M / 256) = 512: no column split
] + [(f, 1, 257, 257, 3, 17, True, "none", kind) for f in FAMS for kind in ("dup", "far")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_wide_product_against_fp64_numpy(case):
    name, B, M, N, D, c, ard, diag, kind = case
    seed = 7000 + 7 * CASES.index(case)
    x1, x2, ls, os_ = make_points(seed, B, M, N, D, ard, kind)
    g = rng(seed + 1)
    v, d = g.standard_normal((B, N, c)).astype(np.float32), (0.05 + g.random((B, N))).astype(np.float32)
    dd = {"none": None, "full": d, "const": d[:, 0]}[diag]
    want = dense64(name, x1, x2, ls, os_) @ v.astype(np.float64)
    fn, tx1, tx2, tv = covariance.FAMILIES[name], dev(x1), dev(x2), dev(v)
    comp = fn(tx1, tx2, dev(ls), dev(os_)) @ tv
    if dd is not None:
        want = want + (d if diag == "full" else d[:, :1])[:, :, None].astype(np.float64) * v
        comp = comp + (dev(dd)[:, :, None] if diag == "full" else dev(dd)[:, None, None]) * tv
    ref_err = max(rel(host(comp), want), ERR_FLOOR)
    if B == 512:
        assert _hip.load().lo_kernel_mv_wide_workspace_bytes(B, M, N, D, c) == 256  # (nothing but the tail: no partials)
    args = (tx1, tx2, theta_of(ls, os_, D), fn.native_family, tv, None if dd is None else dev(dd))
    y = K.kernel_mv_wide(*args, const_diag=diag == "const")
    err = rel(host(y), want)
    print(f"kernel_mv_wide {'-'.join(str(x) for x in case)}: err {err:.3e} torch fp32 {ref_err:.3e} "
          f"ratio {err / ref_err:.2f}")
    assert torch.isfinite(y).all() and err <= REF_FACTOR * ref_err, (case, err, ref_err)
    assert torch.equal(K.kernel_mv_wide(*args, const_diag=diag == "const"), y)  # two calls give equal bits
    if kind == "far":  # only the diagonal survives: y = os^2 v
        assert rel(host(y), os_[:, None, None].astype(np.float64) ** 2 * v) <= 1e-6


def test_wide_entry_point_returns_the_error_codes_of_the_product():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, c = 1, 300, 300, 3, 17
    x, theta = torch.rand(B, M, D, device=DEV), torch.ones(B, D + 1, device=DEV)
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, M, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_mv_wide_workspace_bytes(B, M, N, D, c)  # (> 256: a split member, partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def both(x1=x, dim=D, mode=0, w=ws, wb=need):
        a = (p(x1), p(x), p(theta), 0, B, M, N, dim, p(v), c, None, mode, p(y), p(w), wb, st)
        codes = lib.lo_kernel_mv_wide_f32(*a), lib.lo_kernel_mv_f32(*a)
        assert codes[0] == codes[1], codes
        return codes[0]

    assert both(x1=None) == -1 and both(mode=1) == -1  # LO_ERR_BADARG: a null pointer, a diagonal mode without d
    assert both(dim=33) == _hip.LO_ERR_UNSUPPORTED
    assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: y keeps its fill
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and both() == 0


def test_the_operator_takes_the_wide_kernel_where_the_rule_says_so():
    """The route through kernel_mv_run (one gate: ko_wide), then a preconditioned solve with 17 right-hand sides at
    N = 1013 under the bound of test_public_api_end_to_end_at_n_1013 (4 times the reference's recorded solve error)."""
    c, D = 17, 3  # a cell that ko_wide (csrc/lo_kernel_shape.h) sends to k_kernel_mv_wide
    x1, _, ls, os_ = make_points(7700, 3, 300, 300, D, True)
    tx, tv, td = dev(x1), torch.randn(3, 300, c, device=DEV), 0.1 + torch.rand(3, 300, device=DEV)
    op = KernelLinearOperator(tx, tx, covariance.matern52, num_nonbatch_dimensions=NB, lengthscale=dev(ls),
                              outputscale=dev(os_))
    args = (tx, tx, theta_of(ls, os_, D), covariance.matern52.native_family, tv)
    with no_dense():
        assert torch.equal(op._matmul(tv), K.kernel_mv_wide(*args))
        assert torch.equal(AddedDiagLinearOperator(op, DiagLinearOperator(td))._matmul(tv), K.kernel_mv_wide(*args, td))
    p, G, t = "m52", golden("m52"), tensors("m52")
    rhs = torch.cat((t["rhs"], dev(rng(7701).standard_normal((1, 1013, 16)).astype(np.float32))), -1)
    with solver_settings(settings), no_dense():
        sol = AddedDiagLinearOperator(kernel_op(p, t), DiagLinearOperator(t["noise"])).solve(rhs)
    K64 = torch.from_numpy(dense64("matern52", *(host(t[k]) for k in ("x", "x", "lengthscale", "outputscale")))).to(DEV)
    want = torch.linalg.solve(K64 + torch.diag_embed(t["noise"].double()), rhs.double())
    err, ref_err = rel(host(sol), host(want)), max(float(G["solve_err"]), ERR_FLOOR)
    print(f"kernel_op {p} solve, 17 columns: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err
