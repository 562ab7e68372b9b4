"""CPU tests of the native float64 symmetric eigensolver (csrc/lo_eigh_f64.hip, ABI 36): the two C-ABI symbols, the
sizer, the refusals before any launch, the routing predicate, the pull-backs of functions/_eigh.py through the `impl`
seam (gradcheck and autograd through torch.linalg.eigh), and LinearOperator.eigh / eigvalsh against the reference's
recorded eigenvalues (tests/golden/g44_eigh.npz).  No GPU compute here."""
import ctypes
import os
import re
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from linear_operator_amd import _hip
from linear_operator_amd.functions import _eigh as FE
from linear_operator_amd.operators import DenseLinearOperator, KroneckerProductLinearOperator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_eigh as MG  # noqa: E402

NEW_SYMBOLS = ("lo_eigh_f64_workspace_bytes", "lo_eigh_f64")
FAKE = 0x1000  # a non-null pointer that is never dereferenced: the refusals come before any launch
BIG = 1 << 30


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g44_eigh.npz"))), MG.eigh_inputs()


def test_abi_version_of_library_and_binding():
    assert _hip.ABI_VERSION >= 36
    assert _hip.load().lo_abi_version() == _hip.ABI_VERSION
    assert _hip.LO_EIGH_MAX_N == 1024


def test_the_two_symbols_are_exported_declared_and_bound():
    raw = ctypes.CDLL(_hip.lib_path())
    hdr = open(os.path.join(ROOT, "include", "lo_amd.h")).read()
    declared = set(re.findall(r"\b(lo_[a-z0-9_]+)\s*\(", hdr))
    assert re.search(r"#define\s+LO_EIGH_MAX_N\s+1024\b", hdr)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/lo_amd.h"
        assert name in _hip.EXPORTS and name in _hip._PROTOTYPES, f"{name} missing from _hip._PROTOTYPES"
        assert hasattr(raw, name), f"liblo_amd.so does not export {name}"


def test_sizer():
    lib = _hip.load()
    for B, N in ((3, 300), (1, 1024), (7, 1), (2, 33)):
        with_vec, without = lib.lo_eigh_f64_workspace_bytes(B, N, 1), lib.lo_eigh_f64_workspace_bytes(B, N, 0)
        assert with_vec >= B * N * N * 8
        assert 0 < without <= with_vec
    for wv in (0, 1):
        assert lib.lo_eigh_f64_workspace_bytes(1, 1025, wv) == 0
        assert lib.lo_eigh_f64_workspace_bytes(1, 0, wv) == 0
        assert lib.lo_eigh_f64_workspace_bytes(0, 10, wv) == 0


def test_bad_arguments_are_refused_before_any_launch():
    lib = _hip.load()
    bad = -1  # LO_ERR_BADARG
    assert _hip._ERR[bad] == "bad argument"
    assert lib.lo_eigh_f64(None, FAKE, FAKE, FAKE, 1, 10, 1, FAKE, BIG, None) == bad  # A
    assert lib.lo_eigh_f64(FAKE, None, FAKE, FAKE, 1, 10, 1, FAKE, BIG, None) == bad  # evals
    assert lib.lo_eigh_f64(FAKE, FAKE, FAKE, None, 1, 10, 1, FAKE, BIG, None) == bad  # info
    assert lib.lo_eigh_f64(FAKE, FAKE, None, FAKE, 1, 10, 1, FAKE, BIG, None) == bad  # want_vectors without evecs
    assert lib.lo_eigh_f64(FAKE, FAKE, FAKE, FAKE, 1, 0, 1, FAKE, BIG, None) == bad  # N < 1
    assert lib.lo_eigh_f64(FAKE, FAKE, FAKE, FAKE, -1, 10, 1, FAKE, BIG, None) == bad  # B < 0


def test_sizes_beyond_the_kernel_and_short_workspaces_are_refused_before_any_launch():
    lib = _hip.load()
    assert lib.lo_eigh_f64(FAKE, FAKE, FAKE, FAKE, 1, 1025, 1, FAKE, BIG, None) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_eigh_f64(FAKE, FAKE, None, FAKE, 1, 1025, 0, FAKE, BIG, None) == _hip.LO_ERR_UNSUPPORTED
    short = -3  # LO_ERR_WORKSPACE
    assert _hip._ERR[short] == "workspace too small"
    for wv, evecs in ((1, FAKE), (0, None)):
        need = lib.lo_eigh_f64_workspace_bytes(2, 37, wv)
        assert need >= 2 * 37 * 37 * 8
        assert lib.lo_eigh_f64(FAKE, FAKE, evecs, FAKE, 2, 37, wv, FAKE, need - 1, None) == short
        assert lib.lo_eigh_f64(FAKE, FAKE, evecs, FAKE, 2, 37, wv, None, 0, None) == short
        assert lib.lo_eigh_f64(FAKE, FAKE, evecs, FAKE, 2, 37, wv, None, BIG, None) == short
    # an empty batch is a success that launches nothing
    assert lib.lo_eigh_f64(FAKE, FAKE, FAKE, FAKE, 0, 10, 1, None, 0, None) == 0
    assert lib.lo_eigh_f64(FAKE, FAKE, None, FAKE, 0, 10, 0, None, 0, None) == 0


def test_routing_predicate_keeps_cpu_float32_and_large_matrices_on_aten():
    assert 0 <= FE.EIGH_NATIVE_MAX_N <= 1024 and FE.EIGH_NATIVE_MIN_BATCH >= 1
    with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1):
        assert not FE.native_ok(torch.eye(4, dtype=torch.float64))  # CPU
        assert not FE.native_ok(torch.eye(4, dtype=torch.float32))
        # (device tensors cannot be made here: a meta tensor has the shape and dtype but is not a HIP tensor)
        assert not FE.native_ok(torch.empty(2, 4, 4, dtype=torch.float64, device="meta"))
    fake = mock.Mock(spec=torch.Tensor)  # a stand-in HIP float64 tensor: only the attributes the predicate reads
    fake.is_cuda, fake.dtype = True, torch.float64
    with mock.patch.object(torch, "is_tensor", lambda t: True):
        for n_max, min_b, shape, want in ((64, 1, (3, 64, 64), True), (64, 1, (3, 65, 65), False),
                                          (64, 4, (3, 8, 8), False), (64, 4, (2, 2, 8, 8), True),
                                          (0, 1, (3, 8, 8), False), (64, 1, (3, 8, 9), False),
                                          (4096, 1, (1025, 1025), False)):
            fake.shape = torch.Size(shape)
            fake.dim.return_value = len(shape)
            with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", n_max), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", min_b):
                assert FE.native_ok(fake) is want, (n_max, min_b, shape)
        fake.dtype, fake.shape = torch.float32, torch.Size((3, 8, 8))
        fake.dim.return_value = 3
        with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 64):
            assert not FE.native_ok(fake)
    # the module-level calls keep CPU tensors on ATen, bit for bit
    A = torch.from_numpy(MG.eigh_inputs()["A5"])
    assert all(torch.equal(a, b) for a, b in zip(FE.eigh(A), torch.linalg.eigh(A)))
    assert torch.equal(FE.eigvalsh(A), torch.linalg.eigvalsh(A))


def _torch_eigh(A, want_vectors=True):
    """kernels.eigh restated on float64 torch: the substitute behind the `impl` seam."""
    evals, evecs = torch.linalg.eigh(A)
    return evals, (evecs if want_vectors else None), torch.zeros(A.shape[:-2], dtype=torch.int32)


def _gauge_inputs():
    """N = 6, batch 2, eigenvalues 1, 2, .., 6 scaled per member (distinct, gaps >= 0.5)."""
    g = torch.Generator().manual_seed(36)
    Q, _ = torch.linalg.qr(torch.randn(2, 6, 6, generator=g, dtype=torch.float64))
    lam = torch.arange(1.0, 7.0, dtype=torch.float64) * torch.tensor([[1.0], [0.5]], dtype=torch.float64)
    A = (Q * lam.unsqueeze(-2)) @ Q.mT
    W = torch.randn(2, 6, 6, generator=g, dtype=torch.float64)
    c = torch.randn(2, 6, generator=g, dtype=torch.float64)
    return 0.5 * (A + A.mT), W, c


def _gauge_fn(eigh_fn, W, c):
    """sum(W o Q diag(exp(-l)) Q^T) + sum(c o l): invariant under the sign of every eigenvector."""

    def f(A):
        l, Q = eigh_fn(0.5 * (A + A.mT))
        return (W * ((Q * torch.exp(-l).unsqueeze(-2)) @ Q.mT)).sum() + (c * l).sum()

    return f


def test_eigh_backward_through_the_seam():
    A, W, c = _gauge_inputs()
    with mock.patch.object(FE.impl, "eigh", _torch_eigh):
        f = _gauge_fn(FE.NativeEigh.apply, W, c)
        assert torch.autograd.gradcheck(f, (A.clone().requires_grad_(True),), eps=1e-6, atol=1e-7, rtol=1e-5)
        a1 = A.clone().requires_grad_(True)
        (g1,) = torch.autograd.grad(f(a1), a1)
    a2 = A.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad(_gauge_fn(torch.linalg.eigh, W, c)(a2), a2)
    torch.testing.assert_close(g1, g2, rtol=1e-10, atol=1e-10 * g2.abs().max().item())
    # NativeEigh itself returns a symmetrised gradient, as ATen's eigh does
    with mock.patch.object(FE.impl, "eigh", _torch_eigh):
        a3 = A.clone().requires_grad_(True)
        l, Q = FE.NativeEigh.apply(a3)
        (g3,) = torch.autograd.grad((W * Q).sum() ** 2 + (c * l).sum(), a3)
    a4 = A.clone().requires_grad_(True)
    l, Q = torch.linalg.eigh(a4)
    (g4,) = torch.autograd.grad((W * Q).sum() ** 2 + (c * l).sum(), a4)
    assert torch.equal(g3, g3.mT)
    torch.testing.assert_close(g3, g4, rtol=1e-10, atol=1e-10 * g4.abs().max().item())


def test_eigvalsh_backward_through_the_seam():
    A, _, c = _gauge_inputs()

    def f_of(fn):
        return lambda M: (c * fn(0.5 * (M + M.mT))).sum() + fn(0.5 * (M + M.mT)).pow(2).sum()

    with mock.patch.object(FE.impl, "eigh", _torch_eigh):
        assert torch.autograd.gradcheck(f_of(FE.NativeEigvalsh.apply), (A.clone().requires_grad_(True),), eps=1e-6,
                                        atol=1e-7, rtol=1e-5)
        a1 = A.clone().requires_grad_(True)
        (g1,) = torch.autograd.grad(f_of(FE.NativeEigvalsh.apply)(a1), a1)
    a2 = A.clone().requires_grad_(True)
    (g2,) = torch.autograd.grad(f_of(torch.linalg.eigvalsh)(a2), a2)
    torch.testing.assert_close(g1, g2, rtol=1e-10, atol=1e-10 * g2.abs().max().item())


@pytest.mark.parametrize("n", MG.SIZES)
def test_dense_eigh_and_eigvalsh_match_the_reference(golden, n):
    gold, inp = golden
    A = torch.from_numpy(inp[f"A{n}"])
    op = DenseLinearOperator(A)
    evals, evecs = op.eigh()
    np.testing.assert_allclose(evals.numpy(), gold[f"eigh_evals{n}"], rtol=1e-10)
    np.testing.assert_allclose(op.eigvalsh().numpy(), gold[f"eigvalsh{n}"], rtol=1e-10)
    np.testing.assert_allclose(op.diagonalization(method="symeig")[0].numpy(), gold[f"diag_symeig_evals{n}"], rtol=1e-10)
    Q = evecs.to_dense()
    torch.testing.assert_close(A @ Q, Q * evals.unsqueeze(-2), rtol=0, atol=1e-12 * n)
    # the torch.linalg functions dispatch to the methods
    np.testing.assert_allclose(torch.linalg.eigvalsh(op).numpy(), gold[f"eigvalsh{n}"], rtol=1e-10)
    ev2, q2 = torch.linalg.eigh(op)
    assert isinstance(q2, DenseLinearOperator)
    np.testing.assert_allclose(ev2.numpy(), gold[f"eigh_evals{n}"], rtol=1e-10)


def test_kronecker_eigh_keeps_the_kronecker_structure(golden):
    gold, inp = golden
    factors = [torch.from_numpy(inp[f"K{n}"]) for n in MG.KRON]
    op = KroneckerProductLinearOperator(*(DenseLinearOperator(f) for f in factors))
    evals, evecs = op.eigh()
    assert isinstance(evecs, KroneckerProductLinearOperator)
    assert [tuple(o.shape) for o in evecs.linear_ops] == [(n, n) for n in MG.KRON]
    np.testing.assert_allclose(evals.numpy(), gold["kron_eigh_evals"], rtol=1e-10)
    np.testing.assert_allclose(op.eigvalsh().numpy(), gold["kron_eigvalsh"], rtol=1e-10)
    np.testing.assert_allclose(torch.linalg.eigvalsh(op).numpy(), gold["kron_eigvalsh"], rtol=1e-10)
    Q = evecs.to_dense()
    torch.testing.assert_close(torch.kron(*factors) @ Q, Q * evals.unsqueeze(-2), rtol=0, atol=1e-11)
