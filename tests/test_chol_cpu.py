"""CPU tests of the exact small-N path: CholLinearOperator (class relations, values against the reference fixtures
g31_chol_* through ATen), the new C-ABI symbols, and the backward formulas of the native autograd Functions under
torch.autograd.gradcheck with float64 torch stand-ins for the three kernel wrappers.  No GPU compute here."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from make_golden_chol import SIZES, chol_inputs, sample

from linear_operator_amd import _hip
from linear_operator_amd.functions import _cholesky as FC
from linear_operator_amd.operators import CholLinearOperator, RootLinearOperator, TriangularLinearOperator
from linear_operator_amd.utils.cholesky import psd_safe_cholesky

NEW_SYMBOLS = ("lo_cholesky_workspace_bytes", "lo_cholesky_f32", "lo_tri_solve_f32", "lo_cholesky_solve_f32")


def test_chol_linear_operator_class_relations_match_the_reference():
    L = torch.linalg.cholesky(torch.eye(5) * 2.0 + 0.5)
    C = CholLinearOperator(TriangularLinearOperator(L))
    assert issubclass(CholLinearOperator, RootLinearOperator) and isinstance(C, RootLinearOperator)
    assert isinstance(C.root, TriangularLinearOperator) and C.upper is False
    assert C._cholesky(upper=False) is C.root and C._cholesky(upper=True).upper is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        C2 = CholLinearOperator(L.mT.contiguous(), upper=True)  # a dense tensor: deprecated, orientation detected
    assert any(issubclass(x.category, DeprecationWarning) for x in w)
    assert isinstance(C2.root, TriangularLinearOperator) and C2.root.upper
    with pytest.raises(ValueError, match="lower or upper triangular"):
        CholLinearOperator(torch.ones(3, 3))
    rebuilt = C2.representation_tree()(*C2.representation())
    assert type(rebuilt) is CholLinearOperator and rebuilt.upper and torch.equal(rebuilt.to_dense(), C2.to_dense())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tag,dtype,rtol", [("f64", torch.float64, 1e-5), ("f32", torch.float32, 1e-4)])
def test_chol_linear_operator_reproduces_the_reference_on_cpu(n, tag, dtype, rtol):
    torch.set_num_threads(1)
    g, inp = load_golden(f"g31_chol_n{n}"), chol_inputs()
    at = inp[f"at{n}"]
    A = torch.from_numpy(inp[f"A{n}"]).to(dtype)
    rhs, col = torch.from_numpy(inp[f"rhs{n}"]).to(dtype), torch.from_numpy(inp[f"col{n}"]).to(dtype)

    def close(got, want, what):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        err = np.abs(got - want).max() / np.abs(want).max()
        assert err < rtol, f"{what}: {err:.2e} of max |reference|"

    L = psd_safe_cholesky(A)
    close(sample(L.numpy(), at, n), g[f"L_{tag}"], "factor")
    for upper, F in ((False, L), (True, L.mT.contiguous())):
        o = "up" if upper else "lo"
        C = CholLinearOperator(TriangularLinearOperator(F, upper=upper), upper=upper)
        close(C.solve(rhs).numpy(), g[f"solve_{o}_{tag}"], "solve")
        close(C.solve(col).numpy(), g[f"solve1_{o}_{tag}"], "one-column solve")
        iq, ld = C.inv_quad_logdet(rhs, logdet=True)
        close(iq.numpy(), g[f"iq_{o}_{tag}"], "inv_quad")
        close(ld.numpy(), g[f"ld_{o}_{tag}"], "logdet")
        close(C.inv_quad_logdet(rhs, logdet=False, reduce_inv_quad=False)[0].numpy(), g[f"iqcols_{o}_{tag}"], "inv_quad cols")
        close(sample(C.inverse().to_dense().numpy(), at, n), g[f"inv_{o}_{tag}"], "inverse")
        close(C.to_dense().numpy(), A.numpy(), "to_dense")
        close(C._diagonal().numpy(), A.diagonal(dim1=-2, dim2=-1).numpy(), "diagonal")
        close(C.root_inv_decomposition().to_dense().numpy(), torch.linalg.inv(A.double()).numpy(), "root_inv_decomposition")
    # (the fixtures' gradients are compared on the device, tests/test_gpu_chol.py: the Solve Function's backward is HIP)


def test_binding_and_library_export_the_cholesky_entry_points():
    assert _hip.ABI_VERSION >= 18
    raw = ctypes.CDLL(_hip.lib_path())
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTS, f"{name} missing from _hip._PROTOTYPES"
        assert hasattr(raw, name), f"liblo_amd.so does not export {name}"
    lib = _hip.load()
    assert lib.lo_cholesky_workspace_bytes(3, 300) >= 3 * 320 * 320 * 4
    assert lib.lo_cholesky_workspace_bytes(1, 1025) == 0
    # shapes beyond the kernels are refused before anything is launched (no device needed)
    assert lib.lo_cholesky_f32(0x1000, 0x1000, 0x1000, None, 1, 1025, 0x1000, 1 << 30, None) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_tri_solve_f32(0x1000, 0x1000, 0x1000, None, 1, 1025, 1, 0, 0, None) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_cholesky_solve_f32(0x1000, 0x1000, 0x1000, 1, 1025, 1, 0, None) == _hip.LO_ERR_UNSUPPORTED


def test_native_routing_predicate_keeps_cpu_and_float64_on_aten():
    assert not FC.native_ok(torch.eye(4)) and not FC.native_ok(torch.eye(4, dtype=torch.float64))
    x = FC.substitute(torch.tril(torch.ones(3, 3)), torch.ones(3))  # CPU: torch.linalg.solve_triangular, vector kept
    assert x.shape == (3,) and torch.allclose(x, torch.tensor([1.0, 0.0, 0.0]))


@pytest.fixture
def torch_f64_kernels(monkeypatch):
    """float64 torch implementations behind the seam `functions._cholesky.impl`."""
    def cholesky(A, want_logdet=False):
        L, info = torch.linalg.cholesky_ex(A)
        return L, info

    def triangular_solve(L, rhs, transpose=False, want_sumsq=False, upper=False):
        return torch.linalg.solve_triangular(L.mT if transpose else L, rhs, upper=bool(upper) != bool(transpose))

    def cholesky_solve(L, rhs, upper=False):
        return torch.cholesky_solve(rhs, L, upper=upper)

    monkeypatch.setattr(FC.impl, "cholesky", cholesky)
    monkeypatch.setattr(FC.impl, "triangular_solve", triangular_solve)
    monkeypatch.setattr(FC.impl, "cholesky_solve", cholesky_solve)


def _spd(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(*shape, shape[-1] + 2, generator=g, dtype=torch.float64)
    return X @ X.mT + torch.eye(shape[-1], dtype=torch.float64), g


def test_backward_formulas_pass_gradcheck_in_float64(torch_f64_kernels):
    A, g = _spd(5, 2, 6)
    A.requires_grad_(True)
    # the factorisation is a function of the symmetric matrix: gradcheck perturbs it symmetrically
    assert torch.autograd.gradcheck(lambda M: FC.NativeCholesky.apply(0.5 * (M + M.mT))[0], (A,))
    L = torch.linalg.cholesky(A.detach())
    rhs = torch.randn(2, 6, 3, generator=g, dtype=torch.float64, requires_grad=True)
    shared = torch.randn(6, 2, generator=g, dtype=torch.float64, requires_grad=True)  # batch-less right-hand side
    for upper in (False, True):
        F = (L.mT.contiguous() if upper else L).clone().requires_grad_(True)
        tri = torch.triu if upper else torch.tril
        assert torch.autograd.gradcheck(lambda f, r: FC.NativeCholeskySolve.apply(tri(f), r, upper), (F, rhs))
        assert torch.autograd.gradcheck(lambda f, r: FC.NativeCholeskySolve.apply(tri(f), r, upper), (F, shared))
        for transpose in (False, True):
            assert torch.autograd.gradcheck(lambda f, r: FC.NativeTriSolve.apply(tri(f), r, upper, transpose), (F, rhs))
            assert torch.autograd.gradcheck(lambda f, r: FC.NativeTriSolve.apply(tri(f), r, upper, transpose), (F, shared))
