"""`mul` / `prod` / MulLinearOperator / ConstantMulLinearOperator on the host: the routing of `*`, `/`, `torch.mul` and
`prod` to the reference's classes and the torch compositions (CPU tensors) against the reference's goldens
(tests/golden/g30_mul_*.npz, tests/golden/make_golden_mul.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_mul import MV_RANKS, mul_inputs, run_routing  # noqa: E402

import linear_operator_amd.operators as ops  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    ConstantMulLinearOperator, DenseLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator,
    MulLinearOperator, RootLinearOperator)

X = mul_inputs()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def close(a, b, rel=1e-5):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30)


def test_routing_returns_the_reference_classes():
    got = run_routing(ops, torch, X)
    want = [str(s) for s in golden("g30_mul_routing")["rt_names"]]
    assert got == want


@pytest.mark.parametrize("p,q", MV_RANKS)
@pytest.mark.parametrize("t", [1, 17])
def test_mul_matmul_composition(p, q, t):
    k = f"mv{p}x{q}"
    A = MulLinearOperator(RootLinearOperator(T(X[k + "_F"])), RootLinearOperator(T(X[k + "_G"])))
    y = A._matmul(T(X[f"{k}_rhs{t}"]))
    assert close(y, golden("g30_mul_matvec")[f"{k}_y{t}"])
    assert close(A.to_dense() @ T(X[f"{k}_rhs{t}"]), golden("g30_mul_matvec")[f"{k}_y{t}"], rel=1e-4)


def test_mul_matmul_vector_and_broadcast():
    F, G = T(X["mv7x5_F"]), T(X["mv7x5_G"])
    A = MulLinearOperator(RootLinearOperator(F), RootLinearOperator(G))
    v = T(X["mv7x5_rhs1"])[0, :, 0]
    assert close(A._matmul(v), A.to_dense() @ v, rel=1e-4)


@pytest.mark.parametrize("base", ["dense", "kron", "root"])
def test_constant_mul_matmul(base):
    g = golden("g30_mul_matvec")
    c, rhs = T(X["cm_c"]), T(X["cm_rhs"])
    make = {"dense": lambda: DenseLinearOperator(T(X["cm_K"])),
            "kron": lambda: KroneckerProductLinearOperator(DenseLinearOperator(T(X["cm_K1"])),
                                                           DenseLinearOperator(T(X["cm_K2"]))),
            "root": lambda: RootLinearOperator(T(X["cm_R"]))}[base]
    assert close(ConstantMulLinearOperator(make(), c)._matmul(rhs), g[f"cm_{base}_y"])
    assert close(ConstantMulLinearOperator(make(), c[0])._matmul(rhs), g[f"cm_{base}_y_scalar"])
    cm = ConstantMulLinearOperator(make(), c)
    assert close(cm.to_dense(), make().to_dense() * c[:, None, None])
    assert close(cm._diagonal(), make().to_dense().diagonal(dim1=-1, dim2=-2) * c[:, None])


def test_constant_mul_root_decomposition():
    c = T(X["cm_c"])
    cm = ConstantMulLinearOperator(RootLinearOperator(T(X["cm_R"])), c)
    root = cm.root_decomposition()
    assert isinstance(root, RootLinearOperator) and isinstance(root.root, ConstantMulLinearOperator)
    assert close(root.to_dense(), cm.to_dense(), rel=1e-5)


def test_mul_diagonal_and_indices():
    g = golden("g30_mul_matvec")
    A = MulLinearOperator(RootLinearOperator(T(X["mv7x5_F"])), RootLinearOperator(T(X["mv7x5_G"])))
    assert close(A._diagonal(), g["ix_diag"])
    assert close(A._get_indices(T(X["ix_rows"]), T(X["ix_cols"]), T(X["ix_batch"])), g["ix_vals"])


@pytest.mark.parametrize("k", ["pr2", "pr4"])
def test_prod_over_batch_of_roots(k):
    R = T(X[k + "_R"])
    res = RootLinearOperator(R).prod(-3)
    assert isinstance(res, MulLinearOperator)
    assert close(res.to_dense(), golden("g30_mul_pivchol")[k + "_dense"], rel=1e-4)
    exact = (R @ R.mT).prod(0)
    assert close(res.to_dense(), exact, rel=1e-3)


def test_mul_constant_of_mul_scales_left_root():
    F, G = T(X["mv7x5_F"]), T(X["mv7x5_G"])
    A = MulLinearOperator(RootLinearOperator(F), RootLinearOperator(G))
    B = A * 2.5
    assert isinstance(B, MulLinearOperator) and B.right_linear_op is A.right_linear_op
    assert close(B.to_dense(), 2.5 * A.to_dense(), rel=1e-5)
    assert isinstance(A * -1.0, ConstantMulLinearOperator)


def test_diag_mul_and_sum_distribution():
    d = T(X["rt_d"])
    D = DiagLinearOperator(d)
    assert close((D * 3.0).to_dense(), 3.0 * D.to_dense())
    S = RootLinearOperator(T(X["rt_R"])) + RootLinearOperator(T(X["rt_S"]))
    assert close((S * 0.5).to_dense(), 0.5 * S.to_dense(), rel=1e-5)
    assert close((S / 4).to_dense(), S.to_dense() / 4, rel=1e-5)


def test_mismatched_shapes_raise_the_reference_error():
    A = RootLinearOperator(T(X["rt_R"]))
    with pytest.raises(RuntimeError, match="Cannot multiply LinearOperator of size"):
        A.mul(torch.ones(3, 5, 5))
    with pytest.raises(ValueError, match="only works on batch dimensions"):
        A.prod(-1)
    with pytest.raises(ValueError, match="requires a dim argument"):
        A.prod(None)
