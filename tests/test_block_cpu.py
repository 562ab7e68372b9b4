"""BlockDiagLinearOperator / BlockInterleavedLinearOperator / SumBatchLinearOperator and `LinearOperator.sum` on the host:
shapes, dense forms, products, indexing, solves and gradients of the torch compositions (CPU tensors) against the
reference's goldens (tests/golden/g32_block_*.npz, tests/golden/make_golden_block.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_block import G, KINDS, N, T, block_inputs  # noqa: E402

import linear_operator_amd.operators as ops  # noqa: E402
from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    BlockDiagLinearOperator, BlockInterleavedLinearOperator, BlockLinearOperator, ConstantMulLinearOperator,
    DenseLinearOperator, DiagLinearOperator, SumBatchLinearOperator)

X = block_inputs()
FILES = {"bd": "g32_block_diag", "bi": "g32_block_interleaved", "sb": "g32_block_sum", "sum": "g32_block_sum"}
_GOLD = {}


def Tn(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def gold(key):
    name = FILES[key.split("_")[0]]
    if name not in _GOLD:
        _GOLD[name] = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
    return _GOLD[name][key]


def close(a, b, rel=1e-5):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30)


def make(k, name, base="M", **kw):
    return getattr(ops, name)(DenseLinearOperator(Tn(X[base])), **kw)


@pytest.mark.parametrize("k,name", KINDS)
def test_shape_dense_and_products(k, name):
    A = make(k, name)
    assert isinstance(A, BlockLinearOperator)
    assert tuple(A.shape) == tuple(gold(k + "_shape"))
    assert close(A.to_dense(), gold(k + "_dense"), rel=0)
    r1, r3 = Tn(X[k + "_rhs1"]), Tn(X[k + "_rhs3"])
    assert close(A @ r1, gold(k + "_y1")) and close(A @ r3, gold(k + "_y3"))
    assert close(A._matmul_composition(r3), gold(k + "_y3"))
    assert close(A.mT @ r3, gold(k + "_yT3"))
    assert close(A[0] @ r1[0, :, 0], gold(k + "_yvec"))
    assert close(A[0]._matmul_composition(r1[0, :, 0]), gold(k + "_yvec"))  # (a 1-D vector)


@pytest.mark.parametrize("k,name", KINDS)
def test_diagonal_and_scattered_entries(k, name):
    A = make(k, name)
    assert close(A.diagonal(), gold(k + "_diag"), rel=1e-6)
    pre = "sb" if k == "sb" else "ix"
    b, r, c = (Tn(X[f"{pre}_{s}"]) for s in ("batch", "rows", "cols"))
    vals = A[b, r, c]
    assert close(vals, gold(k + "_vals"), rel=1e-6)
    assert close(A._get_indices(r, c, b), A.to_dense()[b, r, c], rel=1e-6)
    if k != "sb":  # entries off the diagonal blocks are exact zeros
        assert (gold(k + "_vals") == 0).any() and np.array_equal(vals.numpy() == 0, gold(k + "_vals") == 0)


@pytest.mark.parametrize("k,name", KINDS)
def test_indexing(k, name):
    A = make(k, name)
    sub = A[1]
    assert type(sub).__name__ == str(gold(k + "_b1_cls")) == name  # batch-only indexing keeps the blocks
    assert close(sub.to_dense(), gold(k + "_b1_dense"), rel=0)
    assert close(A[:, 4:10, 7:12].to_dense(), gold(k + "_slice"), rel=1e-6)
    assert close(A[0, 5], gold(k + "_row5"), rel=1e-6)


@pytest.mark.parametrize("k,name", KINDS)
def test_block_dim(k, name):
    cls = getattr(ops, name)
    assert close(cls(DenseLinearOperator(Tn(X["M4"])), block_dim=0).to_dense(), gold(k + "_dim0_dense"), rel=0)
    assert close(cls(Tn(X["M4"]), block_dim=-4).to_dense(), gold(k + "_dim0_dense"), rel=0)
    assert close(cls(DenseLinearOperator(Tn(X["M"])), block_dim=-3).to_dense(), gold(k + "_dimm3_dense"), rel=0)
    with pytest.raises(RuntimeError, match="at least 3 dimensions"):
        cls(DenseLinearOperator(Tn(X["M"])[0, 0]))


def test_block_diag_of_diag_is_diag_and_square_blocks_only():
    D = BlockDiagLinearOperator(DiagLinearOperator(Tn(X["dg"])))
    assert type(D).__name__ == str(gold("bd_diagbase_cls")) == "DiagLinearOperator"
    assert close(D.to_dense(), gold("bd_diagbase_dense"), rel=0)
    with pytest.raises(NotImplementedError):
        BlockDiagLinearOperator(DiagLinearOperator(Tn(X["dg"])), block_dim=-2)
    with pytest.raises(RuntimeError, match="square"):
        BlockDiagLinearOperator(Tn(X["M"])[..., :5])
    assert tuple(BlockInterleavedLinearOperator(Tn(X["M"])[..., :5]).shape) == (G, T * N, T * 5)


@pytest.mark.parametrize("k,name", KINDS)
def test_constant_mul_keeps_the_block_structure(k, name):
    S = make(k, name) * Tn(X["c"])
    assert f"{type(S).__name__}/{type(S.base_linear_op).__name__}" == str(gold(k + "_cm_cls"))
    assert isinstance(S.base_linear_op, ConstantMulLinearOperator)
    assert close(S.to_dense(), gold(k + "_cm_dense"), rel=1e-6)
    per_member = make(k, name) * Tn(np.array([2.0, -1.0], np.float32)).view(G, 1, 1)
    assert type(per_member).__name__ == name
    assert close(per_member.to_dense(), make(k, name).to_dense() * Tn(np.array([2.0, -1.0], np.float32)).view(G, 1, 1))


def test_sum_over_every_kind_of_dimension():
    A = DenseLinearOperator(Tn(X["M"]))
    S3, S0 = A.sum(-3), DenseLinearOperator(Tn(X["M4"])).sum(0)
    assert type(S3).__name__ == str(gold("sum_m3_cls")) and type(S0).__name__ == str(gold("sum_0_cls"))
    SR = ops.RootLinearOperator(Tn(X["R"])).sum(-3)
    assert type(SR).__name__ == str(gold("sum_root_cls")) == "SumBatchLinearOperator"
    assert close(SR.to_dense(), gold("sum_root_dense")) and close(SR @ Tn(X["sb_rhs3"]), SR.to_dense() @ Tn(X["sb_rhs3"]))
    assert close(S3.to_dense(), gold("sum_m3_dense")) and close(S0.to_dense(), gold("sum_0_dense"))
    assert close(torch.sum(A, 1).to_dense(), gold("sum_m3_dense"))
    assert close(A._sum_batch(1).to_dense(), SumBatchLinearOperator(A).to_dense())
    assert close(A.sum(-1), gold("sum_m1")) and close(A.sum(-2), gold("sum_m2"))
    assert close(A.sum(), gold("sum_all"))
    with pytest.raises(ValueError, match="Invalid dim"):
        A.sum(4)


@pytest.mark.parametrize("k,name", KINDS[:2])
def test_exact_solve_and_inv_quad_logdet(k, name):
    A = make(k, name, base="K")
    r3 = Tn(X[k + "_rhs3"])
    assert close(A.solve(r3), gold(k + "_solve"), rel=1e-5)
    iq, ld = A.inv_quad_logdet(r3, logdet=True)
    assert close(iq, gold(k + "_iq"), rel=1e-5) and close(ld, gold(k + "_ld"), rel=1e-5)
    dense = A.to_dense().double()
    assert close(ld.double(), torch.logdet(dense), rel=1e-5)
    iq_cols, _ = A.inv_quad_logdet(r3, logdet=False, reduce_inv_quad=False)
    assert close(iq_cols.double(), (r3.double() * torch.linalg.solve(dense, r3.double())).sum(-2), rel=1e-5)
    chol = A.cholesky()
    assert close(chol.to_dense() @ chol.to_dense().mT, A.to_dense(), rel=1e-5)
    assert close(A.root_decomposition().to_dense(), A.to_dense(), rel=1e-5)
    assert close(A.root_inv_decomposition().to_dense().double(), torch.linalg.inv(dense), rel=1e-4)
    evals, evecs = A._symeig(eigenvectors=True)
    assert close((evecs.to_dense() * evals.unsqueeze(-2)) @ evecs.to_dense().mT, A.to_dense(), rel=1e-4)


def test_block_diag_matmul_with_block_diag_and_diag():
    A = make("bd", "BlockDiagLinearOperator")
    P = A @ make("bd", "BlockDiagLinearOperator", base="K2")
    assert type(P).__name__ == str(gold("bd_mm_cls")) == "BlockDiagLinearOperator"
    assert close(P.to_dense(), gold("bd_mm_dense"))
    P = A @ DiagLinearOperator(Tn(X["dg"]).reshape(G, T * N))
    assert type(P).__name__ == str(gold("bd_md_cls"))
    assert close(P.to_dense(), gold("bd_md_dense"))


@pytest.mark.parametrize("k,name", KINDS)
def test_matmul_gradient_matches_the_reference(k, name):
    Mg = Tn(X["M"]).clone().requires_grad_(True)
    (getattr(ops, name)(DenseLinearOperator(Mg)) @ Tn(X[k + "_rhs3"])).sum().backward()
    assert close(Mg.grad, gold(k + "_dM"), rel=1e-5)


@pytest.mark.parametrize("k,name", KINDS[:2])
def test_inv_quad_logdet_gradient_matches_the_reference(k, name):
    Kg = Tn(X["K"]).clone().requires_grad_(True)
    iq, ld = getattr(ops, name)(DenseLinearOperator(Kg)).inv_quad_logdet(Tn(X[k + "_rhs3"]), logdet=True)
    (iq.sum() + ld.sum()).backward()
    assert close(Kg.grad, gold(k + "_dK"), rel=1e-5)


@pytest.mark.parametrize("k,name", KINDS)
def test_batch_transformations(k, name):
    A = make(k, name)
    E = A._expand_batch(torch.Size((4, G)))
    assert type(E).__name__ == name and close(E.to_dense(), A.to_dense().expand(4, *A.shape), rel=0)
    U = A._unsqueeze_batch(0)
    assert close(U.to_dense(), A.to_dense().unsqueeze(0), rel=0)
    P = U._permute_batch(1, 0)
    assert type(P).__name__ == name and close(P.to_dense(), A.to_dense().unsqueeze(1), rel=0)
    samples = make(k, name, base="K").zero_mean_mvn_samples(5)
    assert tuple(samples.shape) == (5, *A.shape[:-1])


def test_binding_exports_the_block_entry_points():
    assert _hip.ABI_VERSION >= 19
    assert "lo_block_mv_workspace_bytes" in _hip.EXPORTS and "lo_block_mv_f32" in _hip.EXPORTS
    assert (_hip.LO_BLOCK_DIAG, _hip.LO_BLOCK_INTERLEAVED, _hip.LO_BLOCK_SUM) == (0, 1, 2)
    assert SumBatchLinearOperator._layout == _hip.LO_BLOCK_SUM
