"""Device tests of the exact small-N path (csrc/lo_chol.hip): the batched factorisation, the triangular and Cholesky
solves, failure semantics, routing of the public entry points away from ATen, gradients and determinism.  Comparators
are float64 on the device.  (Raw batched float32 torch.linalg.cholesky_ex with 256 < n < 384 and batched one-column
torch.cholesky_solve with n > 512 are never called here: they kill the HIP context on this stack.)"""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from make_golden_chol import SIZES, chol_inputs, sample

from linear_operator_amd import kernels as K
from linear_operator_amd import settings
from linear_operator_amd.functions import _cholesky as FC
from linear_operator_amd.operators import CholLinearOperator, DenseLinearOperator, TriangularLinearOperator
from linear_operator_amd.utils.cholesky import psd_safe_cholesky
from linear_operator_amd.utils.errors import NanError, NotPSDError
from linear_operator_amd.utils.warnings import NumericalWarning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR_N = (1, 2, 31, 32, 33, 176, 177, 256, 257, 300, 383, 512, 513, 800, 1024)
BATCHES = ((), (1,), (3,), (2, 2), (130,))
SOLVE_C = (1, 2, 3, 4, 15, 16, 17, 64)


def family(batch, n, seed):
    """A = X X^T + 0.5 I, X [.., n, 24]: the matrices of the Cholesky tests in test_gpu_api.py."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    X = torch.randn(*batch, n, 24, generator=g, device=DEV)
    return X @ X.mT + 0.5 * torch.eye(n, device=DEV), g


def col_err(x, exact):
    return ((x.double() - exact).norm(dim=-2) / exact.norm(dim=-2)).max().item()


@pytest.mark.parametrize("batch", BATCHES, ids=str)
@pytest.mark.parametrize("n", FACTOR_N)
def test_factor_matches_float64(n, batch):
    A, _ = family(batch, n, 1000 + n)
    L, info, logdet = K.cholesky(A, want_logdet=True)
    L64 = torch.linalg.cholesky(A.double())
    err, bar = (L.double() - L64).abs().max().item(), 1e-4 * L64.abs().max().item()
    print(f"n={n} batch={batch}: max |L - L64| = {err:.3e} (bar {bar:.3e})")
    assert L.shape == A.shape and info.shape == A.shape[:-2] and info.dtype == torch.int32
    assert err < bar
    assert torch.count_nonzero(torch.triu(L, 1)).item() == 0
    assert not bool(info.any())
    want = 2 * L64.diagonal(dim1=-2, dim2=-1).log().sum(-1)
    assert logdet.dtype == torch.float64 and torch.allclose(logdet, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("c", SOLVE_C)
@pytest.mark.parametrize("n,batch", [(33, (3,)), (300, (2, 2)), (513, (3,)), (800, ()), (1024, (2,))])
def test_solves_match_float64(n, batch, c):
    A, g = family(batch, n, 2000 + n)
    rhs = torch.randn(*batch, n, c, generator=g, device=DEV)
    L64 = torch.linalg.cholesky(A.double())
    exact = torch.linalg.solve(A.double(), rhs.double())
    for upper, F in ((False, L64.float()), (True, L64.mT.contiguous().float())):
        e = col_err(K.cholesky_solve(F, rhs, upper=upper), exact)
        print(f"n={n} c={c} upper={upper}: cholesky_solve {e:.3e}")
        assert e < 1e-4
        for transpose in (False, True):
            out, sumsq = K.triangular_solve(F, rhs, transpose=transpose, want_sumsq=True, upper=upper)
            M = (F.mT if transpose else F).double()
            want = torch.linalg.solve_triangular(M, rhs.double(), upper=upper != transpose)
            e = col_err(out, want)
            print(f"n={n} c={c} upper={upper} transpose={transpose}: triangular_solve {e:.3e}")
            assert e < 1e-4
            assert torch.allclose(sumsq.double(), (want ** 2).sum(-2), rtol=1e-4, atol=0)
    shared = rhs.reshape(-1, n, c)[0]  # a batch-less right-hand side is broadcast
    assert col_err(K.cholesky_solve(L64.float(), shared), torch.linalg.solve(A.double(), shared.double())) < 1e-4


def test_negative_diagonal_entry_reports_its_minor_and_leaves_the_others():
    A, _ = family((3,), 298, 31)
    A[2, 150, 150] = -1.0
    L, info = K.cholesky(A)
    assert info.tolist() == [0, 0, 151]
    L01, info01 = K.cholesky(A[:2].contiguous())
    assert info01.tolist() == [0, 0] and torch.equal(L[:2], L01)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", NumericalWarning)
        with pytest.raises(NotPSDError):
            psd_safe_cholesky(A)


def test_singular_trailing_block_takes_one_jitter_step():
    P, _ = family((3,), 298, 32)
    A = torch.zeros(3, 300, 300, device=DEV)
    A[:, :298, :298] = P
    A[:, 298, 298] = A[:, 299, 299] = 1.0
    A[1, 298:, 298:] = 1.0
    L, info = K.cholesky(A)
    assert info.tolist() == [0, 300, 0]
    L02, _ = K.cholesky(A[[0, 2]].contiguous())
    assert torch.equal(L[[0, 2]], L02)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        Lj = psd_safe_cholesky(A)
    msgs = [str(x.message) for x in w if issubclass(x.category, NumericalWarning)]
    assert len(msgs) == 1 and "1.0e-06" in msgs[0]
    assert torch.equal(Lj[[0, 2]], L02) and bool(torch.isfinite(Lj).all())


def test_nan_raises_nan_error():
    A, _ = family((2,), 64, 33)
    A[1, 5, 3] = float("nan")
    with pytest.raises(NanError):
        psd_safe_cholesky(A)


@pytest.mark.parametrize("n", [300, 600])
def test_public_entry_points_do_not_reach_aten(n, monkeypatch):
    """solve, inv_quad_logdet, logdet, root_decomposition and CholLinearOperator with torch's factorisation and
    substitution routines made to raise: the exact path is the project's own."""
    A, g = family((3,), n, 4000 + n)
    rhs = torch.randn(3, n, 1, generator=g, device=DEV)
    A64 = A.double()
    exact = torch.linalg.solve(A64, rhs.double())
    want_iq = (rhs.double() * exact).sum((-2, -1))
    want_ld = torch.linalg.slogdet(A64)[1]
    L64 = torch.linalg.cholesky(A64)
    inv64 = torch.linalg.inv(A64)

    def refuse(*a, **k):
        raise AssertionError("the exact path called ATen")

    monkeypatch.setattr(torch.linalg, "cholesky_ex", refuse)
    monkeypatch.setattr(torch, "cholesky_solve", refuse)
    monkeypatch.setattr(torch.linalg, "solve_triangular", refuse)
    op = DenseLinearOperator(A)
    assert col_err(op.solve(rhs), exact) < 1e-4
    iq, ld = op.inv_quad_logdet(rhs, logdet=True)
    assert torch.allclose(iq.double(), want_iq, rtol=1e-4) and torch.allclose(ld.double(), want_ld, rtol=1e-4)
    assert torch.allclose(op.logdet().double(), want_ld, rtol=1e-4)
    R = op.root_decomposition(method="cholesky").root.to_dense()
    assert (R.double() - L64).abs().max().item() < 1e-4 * L64.abs().max().item()
    for upper, F in ((False, L64.float()), (True, L64.mT.contiguous().float()), (True, L64.float().mT)):
        C = CholLinearOperator(TriangularLinearOperator(F, upper=upper), upper=upper)
        assert col_err(C.solve(rhs), exact) < 1e-4
        iq, ld = C.inv_quad_logdet(rhs, logdet=True)
        assert torch.allclose(iq.double(), want_iq, rtol=1e-4) and torch.allclose(ld.double(), want_ld, rtol=1e-4)
        assert torch.allclose(C.inv_quad(rhs).double(), want_iq, rtol=1e-4)
        inv = C.inverse().to_dense().double()
        assert (inv - inv64).abs().max().item() < 1e-4 * inv64.abs().max().item() * n ** 0.5


def _grads(A, rhs, dtype):
    """d/dA of solve(A, rhs).sum() and of inv_quad + logdet through the operator API."""
    out = []
    for which in ("solve", "iql"):
        Ag = A.to(dtype).clone().requires_grad_(True)
        op = DenseLinearOperator(Ag)
        if which == "solve":
            op.solve(rhs.to(dtype)).sum().backward()
        else:
            iq, ld = op.inv_quad_logdet(rhs.to(dtype), logdet=True)
            (iq + ld).sum().backward()
        out.append(Ag.grad.double())
    return out


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("n", SIZES)
def test_gradients_match_the_reference_fixtures(n, monkeypatch):
    """Native float32 gradients against the reference's float64 gradients of g31_chol_*, bar = 4 x the error of the
    ATen float32 path (native routing switched off) on the same inputs.
    Measured on an MI355X, max |g - g_ref| / max |g_ref|, native / ATen: N = 40 solve 5.7e-6 / 3.6e-6,
    inv_quad + logdet 3.7e-6 / 4.3e-6; N = 300 solve 6.4e-5 / 8.9e-5, inv_quad + logdet 5.6e-5 / 7.2e-5."""
    g, inp = load_golden(f"g31_chol_n{n}"), chol_inputs()
    A = torch.from_numpy(inp[f"A{n}"]).to(DEV)
    rhs = torch.from_numpy(inp[f"rhs{n}"]).to(DEV)

    def at_fixture(grads):
        return [torch.from_numpy(sample(x.cpu().numpy(), inp[f"at{n}"], n)) for x in grads]

    native = at_fixture(_grads(A, rhs, torch.float32))
    monkeypatch.setattr(FC, "native_ok", lambda *a, **k: False)
    aten = at_fixture(_grads(A, rhs, torch.float32))
    for nat, at, key in zip(native, aten, ("grad_solve_f64", "grad_iql_f64")):
        want = torch.from_numpy(g[key])
        e_nat, e_at = _rel(nat, want), _rel(at, want)
        print(f"n={n} {key}: native {e_nat:.3e}, ATen {e_at:.3e}")
        assert e_nat <= 4 * e_at


@pytest.mark.parametrize("n", [300, 800])
def test_gradients_within_four_times_the_aten_float32_error(n, monkeypatch):
    """Native float32 gradients against float64 torch autograd of the same expression, bar = 4 x the error of the
    ATen float32 path (the parent's behaviour: native routing switched off) on the same inputs.
    Measured on an MI355X, max |g - g64| / max |g64|, native / ATen: N = 300 solve 7.3e-5 / 8.5e-5,
    inv_quad + logdet 4.3e-5 / 5.8e-5; N = 800 solve 2.2e-4 / 2.5e-4, inv_quad + logdet 1.4e-4 / 1.5e-4."""
    A, g = family((2,), n, 5000 + n)
    rhs = torch.randn(2, n, 3, generator=g, device=DEV)
    want = []
    for which in ("solve", "iql"):
        Ag = A.double().clone().requires_grad_(True)
        x = torch.linalg.solve(Ag, rhs.double())
        ((x.sum()) if which == "solve" else ((rhs.double() * x).sum() + torch.linalg.slogdet(Ag)[1].sum())).backward()
        want.append(0.5 * (Ag.grad + Ag.grad.mT))
    native = [0.5 * (x + x.mT) for x in _grads(A, rhs, torch.float32)]
    monkeypatch.setattr(FC, "native_ok", lambda *a, **k: False)
    aten = [0.5 * (x + x.mT) for x in _grads(A, rhs, torch.float32)]
    for name, nat, at, w in zip(("solve", "inv_quad + logdet"), native, aten, want):
        e_nat, e_at = _rel(nat, w), _rel(at, w)
        print(f"n={n} {name}: native {e_nat:.3e}, ATen {e_at:.3e}")
        assert e_nat <= 4 * e_at


def test_results_repeat_bit_for_bit_and_do_not_depend_on_the_batch():
    A, g = family((130,), 300, 77)
    rhs = torch.randn(130, 300, 5, generator=g, device=DEV)
    L1, _ = K.cholesky(A)
    L2, _ = K.cholesky(A)
    assert torch.equal(L1, L2)
    x1, x2 = K.cholesky_solve(L1, rhs), K.cholesky_solve(L1, rhs)
    y1, s1 = K.triangular_solve(L1, rhs, want_sumsq=True)
    y2, s2 = K.triangular_solve(L1, rhs, want_sumsq=True)
    assert torch.equal(x1, x2) and torch.equal(y1, y2) and torch.equal(s1, s2)
    for k in (0, 57, 129):
        Lk, _ = K.cholesky(A[k].contiguous())
        assert torch.equal(Lk, L1[k])
        assert torch.equal(K.cholesky_solve(Lk, rhs[k].contiguous()), x1[k])


def test_sizes_beyond_the_kernels_keep_the_aten_path():
    A, _ = family((), 1100, 5)
    assert not FC.native_ok(A)
    L = psd_safe_cholesky(A)
    assert (L.double() - torch.linalg.cholesky(A.double())).abs().max().item() < 1e-3
    with pytest.raises(Exception, match="unsupported"):
        K.cholesky(A)
