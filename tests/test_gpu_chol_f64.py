"""Device tests of the float64 exact small-N path (csrc/lo_chol_f64.hip): the batched factorisation, the triangular and
Cholesky solves, the reference's float64 fixtures through the public operators, failure semantics, determinism, routing
away from ATen, and gradients.

Every comparator is computed ON THE CPU in float64 from copies of the inputs, and every bar is a derived backward-error
bound in units of u = 2^-53 (no bar comes from what the kernels give).  Batched one-column torch.cholesky_solve with
n > 512 and batched float32 torch.linalg.cholesky_ex with 256 < n < 384 are never called on the device here: they kill
the HIP context on this stack."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from make_golden_chol import SIZES, chol_inputs, sample

from linear_operator_amd import kernels as K
from linear_operator_amd.functions import _cholesky as FC
from linear_operator_amd.operators import CholLinearOperator, DenseLinearOperator, TriangularLinearOperator
from linear_operator_amd.utils.cholesky import psd_safe_cholesky
from linear_operator_amd.utils.errors import NanError
from linear_operator_amd.utils.warnings import NumericalWarning

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
F64 = torch.float64
FACTOR_N = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 300, 1024)
BATCHES = ((), (1,), (3,), (2, 2))
# the column blocks are 1, 4 and 8 wide: 1 | 2..4 | 5..8 | 9.. (two blocks, the second ragged) | 17 (three blocks)
SOLVE_C = (1, 2, 3, 4, 5, 7, 8, 9, 17)
SOLVE_SHAPES = [(33, (3,)), (300, (2, 2)), (513, (3,)), (1024, (2,))]


def family(batch, n, seed, shift=0.5):
    """A = X X^T + 0.5 I, X [.., n, 24], float64, built on the CPU (the device gets a copy)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(*batch, n, 24, generator=g, dtype=F64)
    return X @ X.mT + shift * torch.eye(n, dtype=F64), g


def factor_residual_excess(A, L):
    """max over the lower triangle of |A - L L^T|_ij / ((2n + 8) u (|L| |L|^T)_ij), on the CPU: at most 1 for a
    factor within Higham's gamma_{n+1} for any summation order, gamma_n for forming the product here, and a few u for
    reciprocal-multiply in place of division."""
    n = A.shape[-1]
    res = torch.tril((A - L @ L.mT).abs())
    bar = (2 * n + 8) * U * torch.tril(L.abs() @ L.abs().mT)
    assert bool((bar.diagonal(dim1=-2, dim2=-1) > 0).all())
    return (res / bar.clamp_min(1e-300)).max().item()


_SOLVE_INPUTS = {}


def solve_inputs(n, batch):
    """(A, L, rhs of 17 columns) on the CPU, once per shape; the tests slice the columns and never modify them."""
    if (n, batch) not in _SOLVE_INPUTS:
        A, g = family(batch, n, 2000 + n)
        _SOLVE_INPUTS[n, batch] = (A, torch.linalg.cholesky(A).contiguous(), torch.randn(*batch, n, max(SOLVE_C), generator=g, dtype=F64))
    return _SOLVE_INPUTS[n, batch]


@pytest.mark.parametrize("n,batch", [(n, b) for n in FACTOR_N for b in BATCHES] + [(33, (130,))], ids=str)
def test_factor_meets_the_backward_error_bound(n, batch):
    A, _ = family(batch, n, 1000 + n)
    L, info, logdet = K.cholesky(A.to(DEV), want_logdet=True)
    assert L.dtype == F64 and L.shape == A.shape and info.shape == A.shape[:-2] and info.dtype == torch.int32
    assert logdet.dtype == F64 and logdet.shape == A.shape[:-2]
    Lc = L.cpu()
    excess = factor_residual_excess(A, Lc)
    want_ld = 2 * Lc.diagonal(dim1=-2, dim2=-1).log().sum(-1)
    ld_err = ((logdet.cpu() - want_ld).abs() / want_ld.abs()).max().item() if want_ld.numel() else 0.0
    print(f"n={n} batch={batch}: residual / bar = {excess:.3f}, logdet rel err = {ld_err:.2e} (bar {4 * n * U:.2e})")
    assert excess <= 1.0
    assert torch.count_nonzero(torch.triu(Lc, 1)).item() == 0
    assert not bool(info.any())
    assert torch.allclose(logdet.cpu(), want_ld, rtol=4 * n * U, atol=0)


def check_tri(F, rhs, x, sumsq, upper, transpose, what):
    n = F.shape[-1]
    tri = torch.triu if upper else torch.tril
    M = tri(F).mT if transpose else tri(F)
    res = (M @ x - rhs).abs()
    bar = 4 * n * U * (M.abs() @ x.abs())
    worst = (res / bar.clamp_min(1e-300)).max().item()
    want_sq = (x ** 2).sum(-2)
    sq_err = ((sumsq - want_sq).abs() / want_sq).max().item()
    print(f"{what}: residual / bar = {worst:.3f}, sumsq rel err = {sq_err:.2e} (bar {4 * n * U:.2e})")
    assert worst <= 1.0, what
    assert torch.allclose(sumsq, want_sq, rtol=4 * n * U, atol=0), what


def check_chol(L, rhs, x, what):
    """|L L^T x - b| <= 8 n u (|L| |L^T| |x|): backward error 2 gamma_n + gamma_n^2, plus this check's two products."""
    n = L.shape[-1]
    res = (L @ (L.mT @ x) - rhs).abs()
    bar = 8 * n * U * (L.abs() @ (L.abs().mT @ x.abs()))
    worst = (res / bar.clamp_min(1e-300)).max().item()
    print(f"{what}: residual / bar = {worst:.3f}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("c", SOLVE_C)
@pytest.mark.parametrize("n,batch", SOLVE_SHAPES)
def test_solves_meet_the_backward_error_bounds(n, batch, c):
    _, L, rhs17 = solve_inputs(n, batch)
    rhs = rhs17[..., :c].contiguous()
    rhs_d = rhs.to(DEV)
    for upper, F in ((False, L), (True, L.mT.contiguous())):
        F_d = F.to(DEV)
        x = K.cholesky_solve(F_d, rhs_d, upper=upper)
        assert x.dtype == F64 and x.shape == rhs.shape
        check_chol(L, rhs, x.cpu(), f"n={n} c={c} upper={upper} cholesky_solve")
        for transpose in (False, True):
            out, sumsq = K.triangular_solve(F_d, rhs_d, transpose=transpose, want_sumsq=True, upper=upper)
            assert out.dtype == F64 and sumsq.dtype == F64 and sumsq.shape == (*batch, c)
            check_tri(F, rhs, out.cpu(), sumsq.cpu(), upper, transpose,
                      f"n={n} c={c} upper={upper} transpose={transpose} triangular_solve")


@pytest.mark.parametrize("n,batch", SOLVE_SHAPES)
def test_shared_right_hand_side_and_transposed_view(n, batch):
    _, L, rhs17 = solve_inputs(n, batch)
    L_d = L.to(DEV)
    shared = rhs17.reshape(-1, n, rhs17.shape[-1])[0, :, :3].contiguous()  # no batch dimensions: broadcast
    x = K.cholesky_solve(L_d, shared.to(DEV))
    assert x.shape == (*batch, n, 3)
    check_chol(L, shared.expand(*batch, n, 3), x.cpu(), f"n={n} shared rhs cholesky_solve")
    out, sumsq = K.triangular_solve(L_d, shared.to(DEV), want_sumsq=True)
    check_tri(L, shared.expand(*batch, n, 3), out.cpu(), sumsq.cpu(), False, False, f"n={n} shared rhs triangular_solve")
    # a transposed view of the contiguous lower factor is an upper factor: handed over with flipped flags, not copied
    view, rhs = L_d.mT, rhs17[..., :5].contiguous()
    assert not view.is_contiguous() and view.mT.is_contiguous()
    x = FC.substitute(view, rhs.to(DEV), upper=True)
    check_tri(L.mT, rhs, x.cpu(), (x.cpu() ** 2).sum(-2), True, False, f"n={n} substitute(view)")
    x = TriangularLinearOperator(view, upper=True)._cholesky_solve(rhs.to(DEV), upper=True)  # (U^T U)^-1 = (L L^T)^-1
    check_chol(L, rhs, x.cpu(), f"n={n} TriangularLinearOperator(view)._cholesky_solve")
    x = K.cholesky_solve(view, rhs.to(DEV), upper=True)
    check_chol(L, rhs, x.cpu(), f"n={n} cholesky_solve(view)")


# ---- the reference's float64 fixtures through the public operators ---------------------------------------------------
def golden_bar(A):
    """2 (3n + 1) n u kappa_2(A): Higham Thm 10.4 with || |L| |L^T| || <= n ||A||, doubled because the reference's own
    result carries the same error.  kappa_2 on the CPU, the largest over the members."""
    n = A.shape[-1]
    return 2 * (3 * n + 1) * n * U * torch.linalg.cond(A.cpu().double()).max().item()


def close(got, want, bar, what):
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"{what}: {err:.2e} (bar {bar:.2e})")
    assert err <= bar, what


def fixture(n):
    g, inp = load_golden(f"g31_chol_n{n}"), chol_inputs()
    A = torch.from_numpy(inp[f"A{n}"]).to(F64)
    rhs, col = torch.from_numpy(inp[f"rhs{n}"]).to(F64), torch.from_numpy(inp[f"col{n}"]).to(F64)
    return g, inp[f"at{n}"], A, rhs, col


@pytest.mark.parametrize("n", SIZES)
def test_reference_fixtures_through_the_public_operators(n):
    g, at, A, rhs, col = fixture(n)
    bar = golden_bar(A)
    assert bar < 1e-6  # four orders below what a float32 computation reaches: a single-precision kernel fails
    A_d, rhs_d, col_d = A.to(DEV), rhs.to(DEV), col.to(DEV)
    L = psd_safe_cholesky(A_d)
    assert L.dtype == F64 and L.is_cuda
    close(sample(L.cpu().numpy(), at, n), g["L_f64"], bar, "factor")
    for upper, F in ((False, L), (True, L.mT.contiguous())):
        o = "up" if upper else "lo"
        C = CholLinearOperator(TriangularLinearOperator(F, upper=upper), upper=upper)
        close(C.solve(rhs_d), g[f"solve_{o}_f64"], bar, f"solve {o}")
        close(C.solve(col_d), g[f"solve1_{o}_f64"], bar, f"one-column solve {o}")
        iq, ld = C.inv_quad_logdet(rhs_d, logdet=True)
        close(iq, g[f"iq_{o}_f64"], bar, f"inv_quad {o}")
        close(ld, g[f"ld_{o}_f64"], bar, f"logdet {o}")
        close(C.inv_quad_logdet(rhs_d, logdet=False, reduce_inv_quad=False)[0], g[f"iqcols_{o}_f64"], bar, f"inv_quad cols {o}")
        close(sample(C.inverse().to_dense().cpu().numpy(), at, n), g[f"inv_{o}_f64"], bar, f"inverse {o}")


# ---- failure semantics ------------------------------------------------------------------------------------------------
def test_negative_diagonal_entry_reports_its_minor_and_leaves_the_others():
    A, _ = family((3,), 40, 31)
    A[1, 17, 17] = -1.0
    A_d = A.to(DEV)
    L, info = K.cholesky(A_d)
    assert info.tolist() == [0, 18, 0]
    for k in (0, 2):
        Lk, infok = K.cholesky(A_d[k].contiguous())
        assert int(infok) == 0 and torch.equal(Lk, L[k])
        assert factor_residual_excess(A[k], Lk.cpu()) <= 1.0


def test_nan_raises_nan_error():
    A, _ = family((2,), 64, 33)
    A[1, 5, 3] = float("nan")
    with pytest.raises(NanError):
        psd_safe_cholesky(A.to(DEV))


def test_rank_deficient_matrix_gets_jitter_and_a_factor_of_the_jittered_matrix():
    A, _ = family((), 40, 34, shift=0.0)  # X X^T of rank 24 < 40
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        L = psd_safe_cholesky(A.to(DEV))
    steps = [x for x in w if issubclass(x.category, NumericalWarning)]
    assert 1 <= len(steps) <= 3
    Aj, prev = A.clone(), 0.0
    for i in range(len(steps)):  # the additions of psd_safe_cholesky, in its order
        new = 1e-8 * 10 ** i
        Aj.diagonal().add_(new - prev)
        prev = new
    assert f"{prev:.1e}" in str(steps[-1].message)
    Lc = L.cpu()
    excess = factor_residual_excess(Aj, Lc)
    print(f"{len(steps)} jitter step(s), residual / bar = {excess:.3f}")
    assert bool(torch.isfinite(Lc).all()) and excess <= 1.0


# ---- determinism -------------------------------------------------------------------------------------------------------
def test_results_repeat_bit_for_bit_and_do_not_depend_on_the_batch():
    A, g = family((130,), 300, 77)
    A = A.to(DEV)
    rhs = torch.randn(130, 300, 5, generator=g, dtype=F64).to(DEV)
    L1, _, ld1 = K.cholesky(A, want_logdet=True)
    L2, _, ld2 = K.cholesky(A, want_logdet=True)
    assert torch.equal(L1, L2) and torch.equal(ld1, ld2)
    x1, x2 = K.cholesky_solve(L1, rhs), K.cholesky_solve(L1, rhs)
    y1, s1 = K.triangular_solve(L1, rhs, want_sumsq=True)
    y2, s2 = K.triangular_solve(L1, rhs, want_sumsq=True)
    assert torch.equal(x1, x2) and torch.equal(y1, y2) and torch.equal(s1, s2)
    for k in (0, 57, 129):
        Lk, _, ldk = K.cholesky(A[k].contiguous(), want_logdet=True)
        assert torch.equal(Lk, L1[k]) and torch.equal(ldk, ld1[k])
        assert torch.equal(K.cholesky_solve(Lk, rhs[k].contiguous()), x1[k])
        yk, sk = K.triangular_solve(Lk, rhs[k].contiguous(), want_sumsq=True)
        assert torch.equal(yk, y1[k]) and torch.equal(sk, s1[k])


# ---- routing -----------------------------------------------------------------------------------------------------------
def test_public_entry_points_do_not_reach_aten(monkeypatch):
    """solve, inv_quad_logdet, cholesky, CholLinearOperator and TriangularLinearOperator on batched float64 device
    inputs at n = 300 with torch's factorisation and substitution routines made to raise."""
    n = 300
    g, at, A, rhs, col = fixture(n)
    bar = golden_bar(A)
    L_cpu = torch.linalg.cholesky(A)
    tri_want = torch.linalg.solve_triangular(L_cpu, rhs, upper=False)
    A_d, rhs_d = A.to(DEV), rhs.to(DEV)
    assert A_d.dim() == 3 and FC.native_ok(A_d) and FC.native_ok(A_d, rhs_d, solve=True)

    def refuse(*a, **k):
        raise AssertionError("the exact path called ATen")

    monkeypatch.setattr(torch.linalg, "cholesky_ex", refuse)
    monkeypatch.setattr(torch, "cholesky_solve", refuse)
    monkeypatch.setattr(torch.linalg, "solve_triangular", refuse)
    op = DenseLinearOperator(A_d)
    close(op.solve(rhs_d), g["solve_lo_f64"], bar, "DenseLinearOperator.solve")
    iq, ld = op.inv_quad_logdet(rhs_d, logdet=True)
    close(iq, g["iq_lo_f64"], bar, "DenseLinearOperator.inv_quad")
    close(ld, g["ld_lo_f64"], bar, "DenseLinearOperator.logdet")
    fac = op.cholesky()
    Lf = fac.factor if hasattr(fac, "factor") else fac.to_dense()
    assert Lf.dtype == F64 and Lf.is_cuda
    close(sample(Lf.cpu().numpy(), at, n), g["L_f64"], bar, "DenseLinearOperator.cholesky")
    for upper, F in ((False, Lf), (True, Lf.mT.contiguous()), (True, Lf.mT)):
        o = "up" if upper else "lo"
        C = CholLinearOperator(TriangularLinearOperator(F, upper=upper), upper=upper)
        close(C.solve(rhs_d), g[f"solve_{o}_f64"], bar, f"CholLinearOperator.solve {o}")
        iq, ld = C.inv_quad_logdet(rhs_d, logdet=True)
        close(iq, g[f"iq_{o}_f64"], bar, f"CholLinearOperator.inv_quad {o}")
        close(ld, g[f"ld_{o}_f64"], bar, f"CholLinearOperator.logdet {o}")
    close(TriangularLinearOperator(Lf).solve(rhs_d), tri_want.numpy(), bar, "TriangularLinearOperator.solve")


def test_sizes_beyond_the_kernels_keep_the_aten_path():
    A, _ = family((), 1100, 5)
    A_d = A.to(DEV)
    assert not FC.native_ok(A_d) and not FC.native_ok(A_d, A_d, solve=True)
    L = psd_safe_cholesky(A_d)
    Lc = L.cpu()
    assert L.dtype == F64 and ((A - Lc @ Lc.mT).norm() / A.norm()).item() < 1e-12
    with pytest.raises(Exception, match="unsupported"):
        K.cholesky(A_d)


def test_mixed_dtypes_raise():
    A, g = family((2,), 40, 6)
    L = torch.linalg.cholesky(A)
    rhs = torch.randn(2, 40, 3, generator=g, dtype=F64)
    L64, L32, r64, r32 = L.to(DEV), L.float().to(DEV), rhs.to(DEV), rhs.float().to(DEV)
    assert FC.native_ok(L64, r64) and FC.native_ok(L32, r32)
    assert not FC.native_ok(L64, r32) and not FC.native_ok(L32, r64)
    for F, r in ((L64, r32), (L32, r64)):
        with pytest.raises(ValueError, match="dtype"):
            K.cholesky_solve(F, r)
        with pytest.raises(ValueError, match="dtype"):
            K.triangular_solve(F, r)
    with pytest.raises(ValueError, match="float32 or float64"):
        K.cholesky(L64.to(torch.float16))


# ---- gradients ---------------------------------------------------------------------------------------------------------
def _spd(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(*shape, shape[-1] + 2, generator=g, dtype=F64)
    return X @ X.mT + torch.eye(shape[-1], dtype=F64), g


@pytest.mark.parametrize("shape", [(2, 6), (33,)], ids=str)
def test_gradcheck_on_the_device_with_the_real_kernels(shape):
    """torch.autograd.gradcheck, default tolerances, with lo_cholesky_f64 / lo_tri_solve_f64 / lo_cholesky_solve_f64
    behind psd_safe_cholesky, chol_solve and tri_solve; n = 33 crosses a 32-row block."""
    n, batch = shape[-1], shape[:-1]
    A, g = _spd(5, *batch, n)
    L = torch.linalg.cholesky(A)
    A_d = A.to(DEV).requires_grad_(True)
    assert FC.native_ok(A_d)
    # the factorisation is a function of the symmetric matrix: gradcheck perturbs it symmetrically
    assert torch.autograd.gradcheck(lambda M: psd_safe_cholesky(0.5 * (M + M.mT)), (A_d,))
    rhs = torch.randn(*batch, n, 2, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    shared = torch.randn(n, 2, generator=g, dtype=F64).to(DEV).requires_grad_(True)  # batch-less right-hand side
    for upper in (False, True):
        F = (L.mT.contiguous() if upper else L).to(DEV).requires_grad_(True)
        tri = torch.triu if upper else torch.tril
        for r in (rhs, shared) if batch else (rhs,):
            assert torch.autograd.gradcheck(lambda f, r: FC.chol_solve(tri(f), r, upper=upper), (F, r))
            for transpose in (False, True):
                assert torch.autograd.gradcheck(lambda f, r: FC.tri_solve(tri(f), r, upper=upper, transpose=transpose), (F, r))


def _grads(A, rhs):
    """d/dA of solve(A, rhs).sum() and of inv_quad + logdet through the operator API."""
    out = []
    for which in ("solve", "iql"):
        Ag = A.clone().requires_grad_(True)
        op = DenseLinearOperator(Ag)
        if which == "solve":
            op.solve(rhs).sum().backward()
        else:
            iq, ld = op.inv_quad_logdet(rhs, logdet=True)
            (iq + ld).sum().backward()
        out.append(Ag.grad)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_gradients_match_the_reference_fixtures(n, monkeypatch):
    g, at, A, rhs, _ = fixture(n)
    bar = golden_bar(A)

    def refuse(*a, **k):
        raise AssertionError("the exact path called ATen")

    monkeypatch.setattr(torch.linalg, "cholesky_ex", refuse)
    monkeypatch.setattr(torch, "cholesky_solve", refuse)
    monkeypatch.setattr(torch.linalg, "solve_triangular", refuse)
    for got, key in zip(_grads(A.to(DEV), rhs.to(DEV)), ("grad_solve_f64", "grad_iql_f64")):
        assert got.dtype == F64
        close(sample(got.cpu().numpy(), at, n), g[key], bar, f"n={n} {key}")
