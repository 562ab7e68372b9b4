"""Device tests of the native float64 batched symmetric eigensolver (csrc/lo_eigh_f64.hip through kernels.eigh and
functions/_eigh.py).  The comparator everywhere is LAPACK through numpy / CPU torch in float64 on copies of the inputs.

Error measures per member, on the CPU, with ulp = 2^-52 (LAPACK's own test ratios):
    r_res  = ||A - Q L Q^T||_1 / (N ulp ||A||_1)        r_orth = ||I - Q^T Q||_1 / (N ulp)
The bar for each is 4 * max(1, the same ratio of numpy's decomposition of that matrix, computed here): 4 is the
project's allowance for a native path against the library, the floor 1 is the N ulp backward-error
scale itself.  Eigenvalues: max_i |l_i - l_i^numpy| <= 2 bar_res N ulp ||A||_1 (Weyl, both backward errors).  No bar is
taken from what the kernel gives; every ratio is printed.

Eigenvalues-only calls run the same scalar recurrence without the vector work: their eigenvalues equal those of the
call with vectors BIT FOR BIT, which is what is asserted."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

from linear_operator_amd import kernels as K
from linear_operator_amd import settings
from linear_operator_amd.functions import _eigh as FE
from linear_operator_amd.operators import (ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator,
                                           KroneckerProductAddedDiagLinearOperator, KroneckerProductDiagLinearOperator,
                                           KroneckerProductLinearOperator, SumKroneckerLinearOperator)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_eigh as MG  # noqa: E402

DEV = "cuda:0"
ULP = 2.0 ** -52
SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 100, 257, 513)
BATCHES = ((), (1,), (3,), (2, 2))
FAMILY_SIZES = (3, 33, 100, 257)
FAMILIES = ("random", "rbf", "repeated", "identity", "diagonal", "blocks", "scaled_up", "scaled_down")


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def sym(x):
    return 0.5 * (x + np.swapaxes(x, -1, -2))


def family(name, n, batch, seed):
    r = rng(seed)
    shape = tuple(batch) + (n, n)
    if name in ("random", "scaled_up", "scaled_down"):
        a = sym(r.standard_normal(shape))
        return a * {"random": 1.0, "scaled_up": 2.0 ** 600, "scaled_down": 2.0 ** -600}[name]
    if name == "rbf":  # the workload: clustered tiny eigenvalues
        x = r.random(tuple(batch) + (n, 2))
        d2 = ((x[..., :, None, :] - x[..., None, :, :]) ** 2).sum(-1)
        return np.exp(-0.5 * d2 / 0.3 ** 2) + 1e-3 * np.eye(n)
    if name == "repeated":
        q, _ = np.linalg.qr(r.standard_normal(shape))
        lam = 1.0 + (np.arange(n) // 4).astype(np.float64)
        return sym((q * lam) @ np.swapaxes(q, -1, -2))
    if name == "identity":
        return np.broadcast_to(np.eye(n), shape).copy()
    if name == "diagonal":
        return r.standard_normal(tuple(batch) + (n,))[..., None] * np.eye(n)
    if name == "blocks":  # an exact zero off-diagonal: deflation
        a = sym(r.standard_normal(shape))
        h = max(1, n // 2)
        a[..., :h, h:] = 0.0
        a[..., h:, :h] = 0.0
        return a
    raise KeyError(name)


def ratios(a, w, q):
    n = a.shape[-1]
    n1 = np.abs(a).sum(0).max()
    res = np.abs(a - (q * w) @ q.T).sum(0).max() / (n * ULP * n1) if n1 > 0 else 0.0
    orth = np.abs(np.eye(n) - q.T @ q).sum(0).max() / (n * ULP)
    return res, orth, n1


def check_members(tag, a_np, w, q):
    """Every member of a_np [*batch, N, N] (symmetric) against numpy's decomposition of it, by the module's bars."""
    n = a_np.shape[-1]
    a3, w3, q3 = a_np.reshape(-1, n, n), w.reshape(-1, n), q.reshape(-1, n, n)
    worst = [0.0, 0.0, 0.0]
    for b in range(a3.shape[0]):
        wr, qr = np.linalg.eigh(a3[b])
        res, orth, n1 = ratios(a3[b], w3[b], q3[b])
        res_np, orth_np, _ = ratios(a3[b], wr, qr)
        bar_res, bar_orth = 4.0 * max(1.0, res_np), 4.0 * max(1.0, orth_np)
        dw = np.abs(w3[b] - wr).max()
        dw_bar = 2.0 * bar_res * n * ULP * n1
        worst = [max(worst[0], res / bar_res), max(worst[1], orth / bar_orth), max(worst[2], dw / dw_bar if dw_bar else 0.0)]
        print(f"eigh {tag} member {b}: r_res {res:.3f} (numpy {res_np:.3f}, bar {bar_res:.2f})  r_orth {orth:.3f} "
              f"(numpy {orth_np:.3f}, bar {bar_orth:.2f})  eigenvalue error / bar {dw / dw_bar if dw_bar else 0.0:.3f}")
        assert np.isfinite(w3[b]).all() and np.isfinite(q3[b]).all(), tag
        assert (np.diff(w3[b]) >= 0).all(), f"{tag}: eigenvalues not ascending"
        assert res <= bar_res, (tag, b, res, bar_res)
        assert orth <= bar_orth, (tag, b, orth, bar_orth)
        assert dw <= dw_bar, (tag, b, dw, dw_bar)
    return worst


def run(a_np, want_vectors=True):
    w, q, info = K.eigh(torch.from_numpy(a_np).to(DEV), want_vectors=want_vectors)
    return w.cpu().numpy(), (q.cpu().numpy() if want_vectors else None), info.cpu().numpy()


def decompose_and_check(tag, a_np):
    w, q, info = run(a_np)
    assert w.shape == a_np.shape[:-1] and q.shape == a_np.shape and info.shape == a_np.shape[:-2]
    assert (info == 0).all(), (tag, info)
    check_members(tag, a_np, w, q)
    w0, q0, info0 = run(a_np, want_vectors=False)
    assert q0 is None and (info0 == 0).all()
    assert np.array_equal(w0, w), f"{tag}: eigenvalues-only differs from the call with vectors"


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_batches(n):
    for batch in BATCHES:
        decompose_and_check(f"random N={n} batch={batch}", family("random", n, batch, 100 * n + len(batch)))


@pytest.mark.parametrize("n,batch", ((33, (130,)), (8, (300,)), (1024, ())))
def test_large_batches_and_the_largest_size(n, batch):
    decompose_and_check(f"random N={n} batch={batch}", family("random", n, batch, 7 * n))


@pytest.mark.parametrize("name", FAMILIES)
def test_families(name):
    for n in FAMILY_SIZES:
        decompose_and_check(f"{name} N={n}", family(name, n, (2,), 31 * n + len(name)))


def test_only_the_lower_triangle_is_read_and_the_input_is_unchanged():
    for n in (3, 33, 100):
        a = family("random", n, (2,), 900 + n)
        w, q, _ = run(a)
        upper_nan = a.copy()
        upper_nan[..., np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
        t = torch.from_numpy(upper_nan).to(DEV)
        keep = t.clone()
        w2, q2, info2 = K.eigh(t)
        assert (info2 == 0).all()
        assert np.array_equal(w2.cpu().numpy(), w) and np.array_equal(q2.cpu().numpy(), q)
        assert torch.equal(torch.nan_to_num(t, nan=7.0), torch.nan_to_num(keep, nan=7.0)), "the input was modified"


def test_results_repeat_and_do_not_depend_on_the_batch():
    for n in (17, 65, 257):
        a = family("rbf", n, (7,), 1200 + n)
        w, q, _ = run(a)
        w2, q2, _ = run(a)
        assert np.array_equal(w, w2) and np.array_equal(q, q2)
        for b in (0, 4):
            wb, qb, _ = run(a[b])
            assert np.array_equal(wb, w[b]) and np.array_equal(qb, q[b]), (n, b)
            wv, _, _ = run(a[b], want_vectors=False)
            assert np.array_equal(wv, w[b])


@pytest.mark.parametrize("poison", (np.nan, np.inf))
def test_a_non_finite_member_fails_alone(poison):
    """An ordinary input the routine must survive: the member's outputs are NaN, info > 0, the others are untouched."""
    n = 33
    a = family("random", n, (3,), 77)
    w, q, _ = run(a)
    bad = a.copy()
    bad[1, 20, 7] = poison  # lower triangle
    for want_vectors in (True, False):
        w2, q2, info2 = run(bad, want_vectors=want_vectors)
        assert info2[1] > 0 and info2[0] == 0 and info2[2] == 0
        assert np.isnan(w2[1]).all()
        assert np.array_equal(w2[0], w[0]) and np.array_equal(w2[2], w[2])
        if want_vectors:
            assert np.isnan(q2[1]).all()
            assert np.array_equal(q2[0], q[0]) and np.array_equal(q2[2], q[2])


def test_wrapper_refuses_what_it_cannot_take():
    with pytest.raises(ValueError):
        K.eigh(torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(Exception):
        K.eigh(torch.zeros(3, 3, dtype=torch.float32, device=DEV))
    w, q, info = K.eigh(torch.zeros(0, 5, 5, dtype=torch.float64, device=DEV))
    assert w.shape == (0, 5) and q.shape == (0, 5, 5) and info.shape == (0,)


# --------------------------------------------------------------------------------------------- routing and consumers
def _no_aten_eigh_on_device():
    """torch.linalg.eigh raising for HIP float64 input: what still runs went through the native route."""
    real = torch.linalg.eigh

    def guarded(A, *args, **kwargs):
        if torch.is_tensor(A) and A.is_cuda and A.dtype == torch.float64:
            raise AssertionError("torch.linalg.eigh was called on a HIP float64 tensor")
        return real(A, *args, **kwargs)

    return mock.patch.object(torch.linalg, "eigh", guarded)


def _spd(seed, batch, n):
    x = rng(seed).standard_normal(tuple(batch) + (n, n))
    return (x @ np.swapaxes(x, -1, -2) / n + 0.5 * np.eye(n)).astype(np.float32)


def _kron64(a, b):
    a, b = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    return (a.unsqueeze(-1).unsqueeze(-3) * b.unsqueeze(-2).unsqueeze(-4)).reshape(
        *a.shape[:-2], a.shape[-2] * b.shape[-2], a.shape[-1] * b.shape[-1])


def _close(value, want, what):
    value, want = value.detach().double().cpu(), want.double()
    err = ((value - want).abs().max() / want.abs().max()).item()
    print(f"eigh consumer {what}: relative error {err:.3e}")
    assert err <= 1e-4, (what, err)


@pytest.mark.parametrize("batch,n1,n2", (((2,), 12, 9), ((1,), 33, 5)))
def test_consumers_run_on_the_native_route(batch, n1, n2):
    dev = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
    a, b, c, d = (_spd(s, batch, n) for s, n in ((1, n1), (2, n2), (3, n1), (4, n2)))
    n = n1 * n2
    rhs = rng(5).standard_normal(tuple(batch) + (n, 3)).astype(np.float32)
    rhs64 = torch.from_numpy(rhs).double()
    kp64 = _kron64(a, b)
    d1 = (0.4 + rng(6).random(tuple(batch) + (n1,))).astype(np.float32)
    d2 = (0.4 + rng(7).random(tuple(batch) + (n2,))).astype(np.float32)
    kp = lambda: KroneckerProductLinearOperator(DenseLinearOperator(dev(a)), DenseLinearOperator(dev(b)))  # noqa: E731
    with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1), \
            _no_aten_eigh_on_device(), settings.max_cholesky_size(0):
        # constant diagonal
        op = kp() + ConstantDiagLinearOperator(torch.full(tuple(batch) + (1,), 0.3, device=DEV), diag_shape=n)
        assert isinstance(op, KroneckerProductAddedDiagLinearOperator)
        full = kp64 + 0.3 * torch.eye(n, dtype=torch.float64)
        _close(op.solve(dev(rhs)), torch.linalg.solve(full, rhs64), "constant diagonal solve")
        _close(op.logdet(), torch.linalg.slogdet(full)[1], "constant diagonal logdet")
        # structured diagonal
        op = kp() + KroneckerProductDiagLinearOperator(DiagLinearOperator(dev(d1)), DiagLinearOperator(dev(d2)))
        assert isinstance(op, KroneckerProductAddedDiagLinearOperator)
        dd = (torch.from_numpy(d1).double().unsqueeze(-1) * torch.from_numpy(d2).double().unsqueeze(-2)).reshape(*batch, n)
        full = kp64 + torch.diag_embed(dd)
        _close(op.solve(dev(rhs)), torch.linalg.solve(full, rhs64), "structured diagonal solve")
        _close(op.logdet(), torch.linalg.slogdet(full)[1], "structured diagonal logdet")
        # sum of two Kronecker products
        op = kp() + KroneckerProductLinearOperator(DenseLinearOperator(dev(c)), DenseLinearOperator(dev(d)))
        assert type(op) is SumKroneckerLinearOperator
        _close(op.solve(dev(rhs)), torch.linalg.solve(kp64 + _kron64(c, d), rhs64), "sum of Kronecker products solve")
    with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1), \
            _no_aten_eigh_on_device():
        evals, evecs = DenseLinearOperator(dev(a)).diagonalization()
        q = evecs.to_dense().double().cpu()
        _close((q * evals.double().cpu().unsqueeze(-2)) @ q.mT, torch.from_numpy(a), "dense diagonalization")
    # the guard itself: with the route closed the same call reaches torch.linalg.eigh and is refused
    with mock.patch.object(FE, "native_ok", lambda A: False), _no_aten_eigh_on_device():
        with pytest.raises(AssertionError):
            DenseLinearOperator(dev(a)).diagonalization()


def test_eigh_of_the_golden_matrices_on_the_device():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "g44_eigh.npz"))
    inp = MG.eigh_inputs()
    with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1), \
            _no_aten_eigh_on_device():
        for n in MG.SIZES:
            a = inp[f"A{n}"]
            atol = 1e-12 * np.abs(a).sum(-2).max()
            op = DenseLinearOperator(torch.from_numpy(a).to(DEV))
            evals, evecs = op.eigh()
            np.testing.assert_allclose(evals.cpu().numpy(), gold[f"eigh_evals{n}"], rtol=1e-10, atol=atol)
            np.testing.assert_allclose(op.eigvalsh().cpu().numpy(), gold[f"eigvalsh{n}"], rtol=1e-10, atol=atol)
            np.testing.assert_allclose(torch.linalg.eigvalsh(op).cpu().numpy(), gold[f"eigvalsh{n}"], rtol=1e-10, atol=atol)
            np.testing.assert_allclose(op.diagonalization(method="symeig")[0].cpu().numpy(),
                                       gold[f"diag_symeig_evals{n}"], rtol=1e-10, atol=atol)
            check_members(f"golden N={n}", a, evals.cpu().numpy(), evecs.to_dense().cpu().numpy())
            np.testing.assert_allclose(FE.eigvalsh(torch.from_numpy(a).to(DEV)).cpu().numpy(), gold[f"eigvalsh{n}"],
                                       rtol=1e-10, atol=atol)
        factors = [torch.from_numpy(inp[f"K{n}"]).to(DEV) for n in MG.KRON]
        kp = KroneckerProductLinearOperator(*(DenseLinearOperator(f) for f in factors))
        evals, evecs = kp.eigh()
        assert isinstance(evecs, KroneckerProductLinearOperator)
        atol = 1e-12 * np.abs(np.kron(inp["K6"], inp["K7"])).sum(-2).max()
        np.testing.assert_allclose(evals.cpu().numpy(), gold["kron_eigh_evals"], rtol=1e-10, atol=atol)
        np.testing.assert_allclose(kp.eigvalsh().cpu().numpy(), gold["kron_eigvalsh"], rtol=1e-10, atol=atol)


def test_gradients_on_the_device():
    """d/dA of sum(W o Q diag(exp(-l)) Q^T) + sum(c o l) (invariant under the eigenvectors' signs) through NativeEigh and
    NativeEigvalsh against autograd through CPU torch.linalg.eigh in float64; N = 40, batch 2, eigenvalue gaps >= 1e-2 by
    construction, so the conditioning of the pull-back is bounded."""
    g = torch.Generator().manual_seed(40)
    n = 40
    q, _ = torch.linalg.qr(torch.randn(2, n, n, generator=g, dtype=torch.float64))
    lam = 0.5 + 0.01 * torch.arange(n, dtype=torch.float64) * torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    A = (q * lam.unsqueeze(-2)) @ q.mT
    A = 0.5 * (A + A.mT)
    W = torch.randn(2, n, n, generator=g, dtype=torch.float64)
    c = torch.randn(2, n, generator=g, dtype=torch.float64)

    def f(eigh_fn, M, W, c):
        l, Q = eigh_fn(0.5 * (M + M.mT))
        return (W * ((Q * torch.exp(-l).unsqueeze(-2)) @ Q.mT)).sum() + (c * l).sum()

    a_ref = A.clone().requires_grad_(True)
    (g_ref,) = torch.autograd.grad(f(torch.linalg.eigh, a_ref, W, c), a_ref)
    a_dev = A.to(DEV).requires_grad_(True)
    (g_dev,) = torch.autograd.grad(f(FE.NativeEigh.apply, a_dev, W.to(DEV), c.to(DEV)), a_dev)
    err = ((g_dev.cpu() - g_ref).abs().max() / g_ref.abs().max()).item()
    print(f"eigh gradient: max|g - g_ref| / max|g_ref| = {err:.3e}")
    assert err <= 1e-8
    a_ref = A.clone().requires_grad_(True)
    (g_ref,) = torch.autograd.grad((c * torch.linalg.eigvalsh(a_ref)).sum(), a_ref)
    a_dev = A.to(DEV).requires_grad_(True)
    with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1):
        (g_dev,) = torch.autograd.grad((c.to(DEV) * FE.eigvalsh(a_dev)).sum(), a_dev)
    err = ((g_dev.cpu() - g_ref).abs().max() / g_ref.abs().max()).item()
    print(f"eigvalsh gradient: max|g - g_ref| / max|g_ref| = {err:.3e}")
    assert err <= 1e-8
