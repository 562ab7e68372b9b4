"""BlockDiag / BlockInterleaved / SumBatch on the MI355X: lo_block_mv_f32 (csrc/lo_block.hip) against fp64 numpy and the
torch composition, its routing from the operators, and the block operators' solves, log-determinants and gradients on
the batched engines of the base operator."""
import itertools
from unittest import mock

import numpy as np
import pytest
import torch

from linear_operator_amd import kernels as K
from linear_operator_amd import settings
from linear_operator_amd.functions import _solve as solve_module
from linear_operator_amd.operators import (
    AddedDiagLinearOperator, BlockDiagLinearOperator, BlockInterleavedLinearOperator, BlockLinearOperator,
    DenseLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator, LowRankRootLinearOperator,
    RootLinearOperator, SumBatchLinearOperator)

pytestmark = pytest.mark.gpu
H = K._hip
LAYOUTS = {"diag": H.LO_BLOCK_DIAG, "interleaved": H.LO_BLOCK_INTERLEAVED, "sum": H.LO_BLOCK_SUM}
CLASSES = {"diag": BlockDiagLinearOperator, "interleaved": BlockInterleavedLinearOperator, "sum": SumBatchLinearOperator}
BAR = 1e-4  # the project's fp32-against-fp64 bar (tests/test_gpu_mul.py); n eps = 1.5e-5 at n = 257 sits inside it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a, b = (host(a) if torch.is_tensor(a) else np.asarray(a)), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def members(seed, G, T, n, R, diag):
    """The base batch [G, T]: dense blocks (R = 0) or roots [G, T, n, R], the diagonal, and the blocks in fp64."""
    r = np.random.default_rng(seed)
    if R == 0:
        A = (r.standard_normal((G, T, n, n)) / np.sqrt(n)).astype(np.float32)
        A64 = A.astype(np.float64)
    else:
        A = (r.standard_normal((G, T, n, R)) / np.sqrt(R)).astype(np.float32)
        A64 = A.astype(np.float64) @ A.astype(np.float64).swapaxes(-1, -2)
    d = None
    if diag == "full":
        d = (0.5 + r.random((G, T, n))).astype(np.float32)
        A64 = A64 + np.einsum("gti,ij->gtij", d.astype(np.float64), np.eye(n))
    elif diag == "const":
        d = (0.5 + r.random((G, T))).astype(np.float32)
        A64 = A64 + d.astype(np.float64)[..., None, None] * np.eye(n)
    return A, d, A64


def block64(layout, A64, v):
    """The product of the block operator in fp64, in the operator's own row order."""
    G, T, n, _ = A64.shape
    v = v.astype(np.float64)
    if layout == "sum":
        return np.einsum("gtij,gjc->gic", A64, v)
    if layout == "diag":
        return np.einsum("gtij,gtjc->gtic", A64, v.reshape(G, T, n, -1)).reshape(G, T * n, -1)
    return np.einsum("gtij,gjtc->gitc", A64, v.reshape(G, n, T, -1)).reshape(G, n * T, -1)


def descriptor(A, d, R, diag):
    fn = K.dense_diag_descriptor if R == 0 else K.lowrank_diag_descriptor
    return fn(dev(A), None if d is None else dev(d), const_diag=(diag == "const"))


@pytest.mark.parametrize("R", [0, 1, 7, 32])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_native_matvec_against_fp64(layout, R):
    worst = 0.0
    for i, (diag, T, n, c, G) in enumerate(itertools.product(("none", "full", "const"), (1, 2, 3, 16), (1, 63, 257),
                                                            (1, 17, 33), (1, 3))):
        A, d, A64 = members(5000 + 7 * i + R, G, T, n, R, diag)
        v = np.random.default_rng(6000 + i).standard_normal((G, n if layout == "sum" else T * n, c)).astype(np.float32)
        y = K.block_matvec(descriptor(A, d, R, diag), LAYOUTS[layout], T, dev(v))
        err = relerr(y, block64(layout, A64, v))
        worst = max(worst, err)
        assert err < BAR, (layout, R, diag, T, n, c, G, err)
    print(f"{layout} R={R}: worst max-norm relative error {worst:.2e}")


@pytest.mark.parametrize("R", [0, 7, 32])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_native_equals_composition(layout, R):
    for i, (diag, T, n, c) in enumerate(itertools.product(("none", "full"), (3, 16), (63, 257), (1, 17))):
        A, d, _ = members(5200 + i + R, 2, T, n, R, diag)
        base = DenseLinearOperator(dev(A)) if R == 0 else RootLinearOperator(dev(A))
        if d is not None:
            base = AddedDiagLinearOperator(base, DiagLinearOperator(dev(d)))
        op = CLASSES[layout](base)
        v = torch.randn(2, op.shape[-1], c, device="cuda")
        y = K.block_matvec(op._native_descriptor(op.batch_shape), LAYOUTS[layout], T, v)
        assert relerr(y, host(op._matmul_composition(v))) < BAR, (layout, R, diag, T, n, c)
        assert relerr(op._matmul(v), host(y)) < BAR


@pytest.mark.parametrize("R", [0, 32])
def test_sum_repeats_bit_for_bit(R):
    A, d, _ = members(5300 + R, 3, 16, 257, R, "full")
    v = dev(np.random.default_rng(5301).standard_normal((3, 257, 17)).astype(np.float32))
    desc = descriptor(A, d, R, "full")
    first = host(K.block_matvec(desc, H.LO_BLOCK_SUM, 16, v))
    assert np.array_equal(first, host(K.block_matvec(desc, H.LO_BLOCK_SUM, 16, v)))


def test_argument_errors_and_unsupported_kinds():
    A, d, _ = members(5400, 1, 6, 9, 0, "none")
    desc = descriptor(A, d, 0, "none")
    with pytest.raises(RuntimeError):
        K.block_matvec(desc, H.LO_BLOCK_SUM, 4, torch.zeros(1, 9, 1, device="cuda"))  # 6 members in groups of 4
    s = desc.c_struct()
    import ctypes as C
    v = torch.zeros(6 * 9, device="cuda")
    assert H.load().lo_block_mv_f32(C.byref(s), H.LO_BLOCK_SUM, 4, H.ptr(v), H.ptr(v.clone()), 1, None, 0,
                                    H.stream_ptr(v.device)) == -1
    kron = K.kron_diag_descriptor(dev(A[0, :, :3, :3]), dev(A[0, :, :3, :3]), None)
    assert K.block_matvec(kron, H.LO_BLOCK_SUM, 3, torch.zeros(2, 9, 1, device="cuda")) is None


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_routing(layout):
    cls = CLASSES[layout]
    A, _, A64 = members(5500, 2, 3, 40, 0, "none")
    rows = 40 if layout == "sum" else 120
    v = np.random.default_rng(5501).standard_normal((2, rows, 2)).astype(np.float32)
    want = block64(layout, A64, v)
    low = cls(LowRankRootLinearOperator(dev(A[..., :5])))
    want_low = block64(layout, A64[..., :5] @ A64[..., :5].swapaxes(-1, -2), v)
    # the shape classes routed to the kernel: BlockDiag always, BlockInterleaved for dense blocks
    # and one column, SumBatch never
    taken = {"diag": (1, 1, 1, 1), "interleaved": (1, 1, 0, 0), "sum": (0, 0, 0, 0)}[layout]
    with mock.patch.object(K, "block_matvec", wraps=K.block_matvec) as spy:
        assert relerr(cls(dev(A))._matmul(dev(v[..., :1])), want[..., :1]) < BAR and spy.call_count == taken[0]
        wt = block64(layout, A64.swapaxes(-1, -2), v)
        assert relerr(cls(dev(A))._t_matmul(dev(v[..., :1])), wt[..., :1]) < BAR
        assert spy.call_count == taken[0] + taken[1]
        assert relerr(cls(dev(A))._matmul(dev(v)), want) < BAR and spy.call_count == sum(taken[:3])
        assert relerr(low._matmul(dev(v[..., :1])), want_low[..., :1]) < BAR and spy.call_count == sum(taken)
    with mock.patch.object(K, "block_matvec", side_effect=AssertionError("native path taken")):
        assert relerr(cls(dev(A).double())._matmul(dev(v).double()), want) < 1e-12  # fp64
        one = cls(dev(A)[0])
        assert relerr(one._matmul(dev(v)[0, :, 0]), want[0, :, 0]) < BAR  # a 1-D vector
        k1, k2 = dev(A[..., :8, :8]), dev(A[..., :5, :5])  # a Kronecker base
        kron = cls(KroneckerProductLinearOperator(DenseLinearOperator(k1), DenseLinearOperator(k2)))
        K64 = np.einsum("gtab,gtcd->gtacbd", A64[..., :8, :8], A64[..., :5, :5]).reshape(2, 3, 40, 40)
        assert relerr(kron._matmul(dev(v)), block64(layout, K64, v)) < BAR


def _lowrank_blocks(seed):
    r = np.random.default_rng(seed)
    C = (r.standard_normal((2, 4, 2048, 8)) / np.sqrt(8)).astype(np.float32)
    d = (0.5 + 0.5 * r.random((2, 4, 2048))).astype(np.float32)
    return C, d


@pytest.mark.parametrize("layout", ["diag", "interleaved"])
def test_solve_is_one_batched_solve_of_the_base(layout):
    C, d = _lowrank_blocks(5600)
    rhs = np.random.default_rng(5601).standard_normal((2, 4 * 2048, 2)).astype(np.float32)
    base = AddedDiagLinearOperator(LowRankRootLinearOperator(dev(C)), DiagLinearOperator(dev(d)))
    op = CLASSES[layout](base)
    calls = []
    real = solve_module._solve

    def counted(linear_op, cols):
        calls.append(linear_op)
        return real(linear_op, cols)

    with mock.patch.object(solve_module, "_solve", side_effect=counted), \
            settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        x = op.solve(dev(rhs))
    base_calls = [c for c in calls if not isinstance(c, BlockLinearOperator)]
    assert len(base_calls) == 1 and tuple(base_calls[0].batch_shape) == (2, 4)
    A64 = C.astype(np.float64) @ C.astype(np.float64).swapaxes(-1, -2)
    A64 += np.einsum("gti,ij->gtij", d.astype(np.float64), np.eye(2048))
    r64 = rhs.astype(np.float64)
    cols = r64.reshape(2, 4, 2048, 2) if layout == "diag" else r64.reshape(2, 2048, 4, 2).swapaxes(1, 2)
    want = np.linalg.solve(A64, cols)
    want = want.reshape(2, 8192, 2) if layout == "diag" else want.swapaxes(1, 2).reshape(2, 8192, 2)
    assert np.allclose(host(x), want, rtol=1e-3, atol=1e-3 * np.abs(want).max())


def test_joint_cg_runs_on_the_native_interleaved_product():
    r = np.random.default_rng(5700)
    a = r.standard_normal((3, 400, 400))
    blocks = (a @ a.swapaxes(-1, -2) / 400).astype(np.float32)
    d = (0.5 + 0.5 * r.random(1200)).astype(np.float32)
    rhs = r.standard_normal((1200, 1)).astype(np.float32)  # (one column: the product every CG iteration makes)
    op = AddedDiagLinearOperator(BlockInterleavedLinearOperator(dev(blocks)), DiagLinearOperator(dev(d)))
    assert op.size(-1) > settings.max_cholesky_size.value()
    with mock.patch.object(K, "block_matvec", wraps=K.block_matvec) as spy, \
            settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        x = op.solve(dev(rhs))
    assert spy.call_count > 0
    full = np.zeros((400, 3, 400, 3))
    for t in range(3):
        full[:, t, :, t] = blocks[t].astype(np.float64)
    full = full.reshape(1200, 1200) + np.diag(d.astype(np.float64))
    want = np.linalg.solve(full, rhs.astype(np.float64))
    assert np.allclose(host(x), want, rtol=1e-3, atol=1e-3 * np.abs(want).max())


def test_exact_path_of_large_block_diag():
    r = np.random.default_rng(5800)
    a = r.standard_normal((4, 300, 300))
    blocks = (a @ a.swapaxes(-1, -2) / 300 + np.eye(300)).astype(np.float32)
    rhs = r.standard_normal((1200, 3)).astype(np.float32)
    op = BlockDiagLinearOperator(dev(blocks))
    from linear_operator_amd.functions import _cholesky as FC

    with mock.patch.object(FC.impl, "cholesky", wraps=FC.impl.cholesky) as spy:
        iq, ld = op.inv_quad_logdet(dev(rhs), logdet=True)
    assert spy.call_count >= 1  # the blocks are factorised by the native batched Cholesky
    b64, r64 = blocks.astype(np.float64), rhs.astype(np.float64).reshape(4, 300, 3)
    want_ld = np.linalg.slogdet(b64)[1].sum()
    want_iq = (r64 * np.linalg.solve(b64, r64)).sum()
    assert torch.allclose(iq.double().cpu(), torch.tensor(want_iq), rtol=1e-4)
    assert torch.allclose(ld.double().cpu(), torch.tensor(want_ld), rtol=1e-4)


@pytest.mark.parametrize("R", [0, 6])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_matmul_gradient(layout, R):
    A, _, _ = members(5900 + R, 2, 3, 70, R, "none")
    rows = 70 if layout == "sum" else 210
    v = np.random.default_rng(5901).standard_normal((2, rows, 3)).astype(np.float32)
    w = np.random.default_rng(5902).standard_normal((2, rows, 3)).astype(np.float32)
    At = dev(A).requires_grad_(True)
    op = CLASSES[layout](DenseLinearOperator(At) if R == 0 else RootLinearOperator(At))
    ((op @ dev(v)) * dev(w)).sum().backward()
    A64 = torch.from_numpy(A.astype(np.float64)).requires_grad_(True)
    dense = CLASSES[layout](A64 if R == 0 else A64 @ A64.mT).to_dense()
    ((dense @ torch.from_numpy(v.astype(np.float64))) * torch.from_numpy(w.astype(np.float64))).sum().backward()
    assert relerr(At.grad, A64.grad.numpy()) < BAR


@pytest.mark.parametrize("R", [0, 6])
@pytest.mark.parametrize("layout", ["diag", "interleaved"])
def test_solve_gradient(layout, R):
    r = np.random.default_rng(5950 + R)
    if R == 0:
        a = r.standard_normal((2, 3, 70, 70))
        A = (a @ a.swapaxes(-1, -2) / 70 + np.eye(70)).astype(np.float32)
    else:
        A = (r.standard_normal((2, 3, 70, R)) / np.sqrt(R)).astype(np.float32)
    d = (0.5 + r.random((2, 3, 70))).astype(np.float32)
    rhs = r.standard_normal((2, 210, 2)).astype(np.float32)
    At = dev(A).requires_grad_(True)
    base = DenseLinearOperator(At) if R == 0 else AddedDiagLinearOperator(RootLinearOperator(At),
                                                                         DiagLinearOperator(dev(d)))
    x = CLASSES[layout](base).solve(dev(rhs))
    (x * dev(rhs)).sum().backward()
    A64 = torch.from_numpy(A.astype(np.float64)).requires_grad_(True)
    blocks = A64 if R == 0 else A64 @ A64.mT + torch.diag_embed(torch.from_numpy(d.astype(np.float64)))
    r64 = torch.from_numpy(rhs.astype(np.float64))
    x64 = torch.linalg.solve(CLASSES[layout](blocks).to_dense(), r64)
    (x64 * r64).sum().backward()
    assert relerr(x, x64.detach().numpy()) < BAR and relerr(At.grad, A64.grad.numpy()) < BAR
