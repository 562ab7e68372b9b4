"""The float64 many-column product of the matrix-free kernel operator on the MI355X: lo_kernel_mv_wide_f64
(csrc/lo_kernel_mv_wide_f64.hip, kernel values on the vector ALU, their product with V on v_mfma_f64_16x16x4_f64) against
the numpy longdouble truth of tests/kernel_f64_cases.py.  The bound is the one of tests/test_gpu_kernel_f64.py: at most
REF_FACTOR = 4 times max(the error of the torch float64 composition on the same inputs, 2^-52); every case prints its
ratio."""
import warnings
from unittest import mock

import numpy as np
import pytest
import torch

from test_gpu_kernel_f64 import (CG_TOLERANCE, DEV, F64, T, dev, diag_of, host, kernel_op, problem, rng, solver_settings,
                                 theta_of, within_bound)
from kernel_f64_cases import FLOOR, REF_FACTOR, rel

from linear_operator_amd import _hip, covariance, settings
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator
from linear_operator_amd.operators.added_diag_linear_operator import clear_preconditioner_memo

pytestmark = pytest.mark.gpu

# (family, B, M, N, D, c, ARD, diagonal); M == N: x2 is x1.  M: a 16-row tile (1, 15, 17), a wave (63, 65), a row block
# (257); N: a ragged last MFMA step of four points (1, 2, 3, 5), the 128-point tile and js > 1 (127, 129); c: one, two and
# three column tiles and a ragged last sweep (1, 15, 16, 17, 33, 65); every family meets every padded dimension.
CASES = [
    ("rbf", 1, 1, 1, 1, 1, False, "full"), ("rbf", 3, 15, 127, 8, 15, True, "none"),
    ("rbf", 1, 257, 257, 16, 17, False, "const"), ("rbf", 1, 65, 129, 32, 33, True, "none"),
    ("rbf", 1, 17, 5, 3, 65, True, "none"), ("rbf", 1, 257, 257, 32, 65, True, "full"),
    ("matern12", 1, 129, 129, 3, 65, True, "full"), ("matern12", 1, 257, 2, 8, 1, False, "none"),
    ("matern12", 3, 63, 129, 16, 16, True, "none"), ("matern12", 1, 1, 127, 17, 17, False, "none"),
    ("matern12", 1, 127, 127, 32, 33, True, "const"), ("matern12", 1, 257, 257, 8, 33, False, "none"),
    ("matern32", 1, 65, 1, 1, 33, True, "none"), ("matern32", 1, 3, 3, 8, 65, False, "const"),
    ("matern32", 1, 15, 129, 16, 1, True, "none"), ("matern32", 3, 257, 257, 17, 15, False, "full"),
    ("matern32", 1, 17, 3, 3, 17, True, "none"),
    ("matern52", 1, 257, 127, 1, 33, False, "none"), ("matern52", 1, 5, 5, 8, 33, True, "full"),
    ("matern52", 1, 65, 257, 16, 65, False, "none"), ("matern52", 3, 63, 3, 32, 1, True, "none"),
    ("matern52", 1, 257, 257, 3, 16, False, "const"),
    ("rbf", 3, 130, 77, 3, 17, True, "none"), ("matern52", 1, 77, 130, 8, 17, False, "none"),
    ("matern32", 512, 33, 129, 3, 17, True, "none"),  # B ceil(M / 256) = 512: no column split
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_wide_f64_product_against_longdouble(case):
    name, B, M, N, D, c, ard, mode = case
    seed, same = 9000 + 7 * CASES.index(case), M == N
    x1, x2, ls, os_ = problem(seed, B, M, N, D, ard, same)
    v = rng(seed + 1).standard_normal((B, N, c))
    dn, dt, const = diag_of(mode, B, N, seed + 2)
    theta = theta_of(ls, os_, B, D)
    truth = T.dense_ld(name, x1, x2, host(theta)) @ v.astype(T.LD)
    t1, tv = dev(x1), dev(v)
    t2 = t1 if same else dev(x2)
    ref = covariance.FAMILIES[name](t1, t2, dev(ls), dev(os_)) @ tv
    if dn is not None:
        truth = truth + dn.astype(T.LD) * v
        ref = ref + dev(np.broadcast_to(dn, (B, N, 1)).copy()) * tv
    if B == 512:
        assert _hip.load().lo_kernel_mv_wide_f64_workspace_bytes(B, M, N, D, c) == 256  # (the tail: no partials)
    args = (t1, t2, theta, T.FAMILY_CODES[name], tv, dt, const)
    y = K.kernel_mv_wide(*args)
    assert y.dtype == F64 and tuple(y.shape) == (B, M, c)
    within_bound("mv_wide " + "-".join(str(x) for x in case), y, truth, ref)
    assert torch.equal(K.kernel_mv_wide(*args), y)  # two calls give equal bits


def test_wide_f64_entry_point_returns_the_error_codes_of_the_product():
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, c = 1, 300, 300, 3, 17
    x, theta = torch.rand(B, M, D, dtype=F64, device=DEV), torch.ones(B, D + 1, dtype=F64, device=DEV)
    v, y = torch.randn(B, N, c, dtype=F64, device=DEV), torch.full((B, M, c), -7.0, dtype=F64, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_mv_wide_f64_workspace_bytes(B, M, N, D, c)  # (> 256: a split member, partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def both(x1=x, dim=D, mode=0, w=ws, wb=need):
        a = (p(x1), p(x), p(theta), 0, B, M, N, dim, p(v), c, None, mode, p(y), p(w), wb, st)
        codes = lib.lo_kernel_mv_wide_f64(*a), lib.lo_kernel_mv_f64(*a)
        assert codes[0] == codes[1], codes
        return codes[0]

    assert need > 256 and both(x1=None) == -1 and both(mode=1) == -1  # a null pointer, a diagonal mode without d
    assert both(dim=33) == _hip.LO_ERR_UNSUPPORTED
    assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: y keeps its fill
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and both() == 0


def test_the_f64_operator_takes_the_wide_kernel_where_the_rule_says_so(monkeypatch):
    """The route through kernel_mv_run_f64 (one gate: ko64_wide), alone, with a diagonal and as the terms of a float64
    LO_OP_SUM (whose second term accumulates), then a preconditioned solve with 17 right-hand sides at N = 300 against
    torch.linalg.solve, within 4 times the error of the parent's route (covar_func densely) on the same inputs."""
    B, N, D, c = 3, 300, 3, 17  # a cell that ko64_wide (csrc/lo_kernel_shape.h) sends to k64_kernel_mv_wide
    x1, _, ls, os_ = problem(9700, B, N, N, D, True, same=True)
    _, _, ls2, os2 = problem(9701, B, N, N, D, False, same=True)
    v, noise = rng(9702).standard_normal((B, N, c)), 0.05 + 0.1 * rng(9703).random((B, N))
    tx, tv, td = dev(x1), dev(v), dev(noise)
    th1, th2 = theta_of(ls, os_, B, D), theta_of(ls2, os2, B, D)
    k1 = kernel_op("matern52", tx, tx, dev(ls), dev(os_))
    k2 = kernel_op("rbf", tx, tx, dev(ls2), dev(os2))
    A = AddedDiagLinearOperator(k1, DiagLinearOperator(td))
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        assert torch.equal(k1._matmul(tv), K.kernel_mv_wide(tx, tx, th1, 3, tv))
        assert torch.equal(A._matmul(tv), K.kernel_mv_wide(tx, tx, th1, 3, tv, td))
        S = (k1 + k2) + DiagLinearOperator(td)
        assert S._kernel_descriptor().kind == _hip.LO_OP_SUM
        truth = (T.dense_ld("matern52", x1, x1, host(th1)) + T.dense_ld("rbf", x1, x1, host(th2))) @ v.astype(T.LD)
        ref = (covariance.matern52(tx, tx, dev(ls), dev(os_)) + covariance.rbf(tx, tx, dev(ls2), dev(os2))) @ tv
        within_bound("Kernel + Kernel + Diag matmul, 17 columns", S._matmul(tv),
                     truth + noise[:, :, None] * v, ref + td[:, :, None] * tv)

    def solve(shut):
        clear_preconditioner_memo()
        with monkeypatch.context() as mp, solver_settings(settings), settings.cg_tolerance(CG_TOLERANCE), \
                warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if shut:
                mp.setattr(KernelLinearOperator, "_native_f64_refusal", lambda self, check_device=True: "shut")
            return A.solve(tv)

    want = torch.linalg.solve(covariance.matern52(tx, tx, dev(ls), dev(os_)) + torch.diag_embed(td), tv)
    err, ref_err = rel(host(solve(False)), host(want)), max(rel(host(solve(True)), host(want)), FLOOR)
    clear_preconditioner_memo()
    print(f"kernel_f64 solve, 17 columns: err {err:.3e} parent's route {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err
