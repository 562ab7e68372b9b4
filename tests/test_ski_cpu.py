"""Toeplitz / interpolated (SKI) operators on CPU tensors against the reference's goldens (tests/golden/g29_ski_*.npz,
made by tests/golden/make_golden_ski.py).  No GPU: the torch compositions of utils/toeplitz.py and
utils/interpolation.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import ski_inputs  # noqa: E402

from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
    ToeplitzLinearOperator)

X = ski_inputs()
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def ski(p, right=True):
    r = (T(X[p + "_ri"]), T(X[p + "_rv"])) if right else (T(X[p + "_li"]), T(X[p + "_lv"]))
    return InterpolatedLinearOperator(ToeplitzLinearOperator(T(X[p + "_col"])), T(X[p + "_li"]), T(X[p + "_lv"]), *r)


def test_toeplitz_against_golden():
    g = golden("g29_ski_toeplitz")
    tz = ToeplitzLinearOperator(T(X["tz_col"]))
    assert np.allclose(tz._matmul(T(X["tz_rhs"])).numpy(), g["tz_matmul"], rtol=1e-4, atol=1e-5)
    assert np.array_equal(tz._diagonal().numpy(), g["tz_diag"])
    assert np.allclose(tz.to_dense().numpy(), g["tz_dense"], rtol=1e-5, atol=1e-6)
    bil = tz._bilinear_derivative(T(X["tz_u"]), T(X["tz_v"]))[0]
    assert bil.shape == tz.column.shape
    assert np.allclose(bil.numpy(), g["tz_bil"], rtol=1e-4, atol=1e-3)


def test_interpolated_against_golden():
    g = golden("g29_ski_interp")
    rows = torch.tensor([0, 5, 99, 42]), torch.tensor([3, 5, 0, 77])
    for J in (4, 16):
        p = f"sq{J}"
        A = ski(p)
        rhs = T(X[p + "_rhs"])
        assert np.allclose(A._matmul(rhs).numpy(), g[p + "_matmul"], rtol=1e-4, atol=1e-5)
        assert np.allclose(A._t_matmul(rhs).numpy(), g[p + "_tmatmul"], rtol=1e-4, atol=1e-5)
        assert np.allclose(A.matmul(rhs).numpy(), g[p + "_mm"], rtol=1e-4, atol=1e-5)
        assert np.allclose(A._approx_diagonal().numpy(), g[p + "_approx_diag"], rtol=1e-6)
        assert np.allclose(A._diagonal().numpy(), g[p + "_diag"], rtol=1e-5, atol=1e-6)
        assert np.allclose(A._get_indices(rows[0], rows[1], torch.tensor([0, 1, 1, 0])).numpy(), g[p + "_getidx"],
                           rtol=1e-5, atol=1e-6)
    A = ski("re")
    assert A.shape == (2, 70, 100)
    assert np.allclose(A._matmul(T(X["re_rhs"])).numpy(), g["re_matmul"], rtol=1e-4, atol=1e-5)
    assert np.allclose(A._t_matmul(T(X["re_lhs"])).numpy(), g["re_tmatmul"], rtol=1e-4, atol=1e-5)
    assert np.allclose(A.matmul(T(X["re_rhs"])).numpy(), g["re_mm"], rtol=1e-4, atol=1e-5)
    bil = A._bilinear_derivative(T(X["re_lhs"]), T(X["re_rhs"]))
    assert len(bil) == 5 and bil[1].dtype == torch.int64 and bil[3].dtype == torch.int64
    for got, key in ((bil[0], "re_bil_col"), (bil[2], "re_bil_lv"), (bil[4], "re_bil_rv")):
        assert np.allclose(got.numpy(), g[key], rtol=1e-4, atol=1e-4), key


def test_diag_shortcut_and_samples():
    A = ski("sq4")
    d = torch.rand(2, 100) + 0.5
    B = A.matmul(DiagLinearOperator(d))
    assert isinstance(B, InterpolatedLinearOperator)
    assert torch.allclose(B.to_dense(), A.to_dense() * d.unsqueeze(-2), rtol=1e-4, atol=1e-5)
    tz = ToeplitzLinearOperator(T(X["sq4_col"]))
    assert torch.allclose(tz._mul_constant(2.0).to_dense(), 2.0 * tz.to_dense())
    assert torch.allclose(A._mul_constant(3.0).to_dense(), 3.0 * A.to_dense(), rtol=1e-5, atol=1e-5)
    k = torch.tensor([2.0, 0.5])  # one constant per batch member
    assert torch.allclose(tz._mul_constant(k).to_dense(), k.view(2, 1, 1) * tz.to_dense())
    assert torch.allclose(A._mul_constant(k).to_dense(), k.view(2, 1, 1) * A.to_dense(), rtol=1e-5, atol=1e-5)


def test_to_keeps_int64_indices():
    A = ski("sq4").to(torch.float64)
    assert A.left_interp_indices.dtype == torch.int64 and A.right_interp_indices.dtype == torch.int64
    assert A.left_interp_values.dtype == torch.float64 and A.base_linear_op.column.dtype == torch.float64
    assert torch.allclose(A.to_dense(), ski("sq4").to_dense().double(), rtol=1e-5, atol=1e-6)


def test_detach_and_representation_roundtrip():
    A = ski("sq16")
    reps = A.representation()
    assert len(reps) == 5
    B = A.representation_tree()(*reps)
    assert isinstance(B, InterpolatedLinearOperator)
    rhs = T(X["sq16_rhs"])
    assert torch.equal(B._matmul(rhs), A._matmul(rhs))
    C = A.detach()
    assert torch.equal(C._matmul(rhs), A._matmul(rhs))
    Ad = AddedDiagLinearOperator(A, DiagLinearOperator(torch.ones(2, 100)))
    Bd = Ad.representation_tree()(*Ad.representation())
    assert torch.allclose(Bd._matmul(rhs), Ad._matmul(rhs))


def test_install_as_exposes_modules():
    """Runs in a subprocess (as test_host_api's install_as test): the alias must not leak into the other tests."""
    import subprocess
    import textwrap

    code = textwrap.dedent("""
        import importlib, sys
        sys.path.insert(0, %r)
        import linear_operator_amd
        assert "linear_operator" not in sys.modules
        linear_operator_amd.install_as("linear_operator")
        for name in ("linear_operator.operators.toeplitz_linear_operator",
                     "linear_operator.operators.interpolated_linear_operator",
                     "linear_operator.utils.toeplitz", "linear_operator.utils.interpolation"):
            mod = importlib.import_module(name)
            assert mod is sys.modules["linear_operator_amd" + name[len("linear_operator"):]], name
        from linear_operator.operators import InterpolatedLinearOperator, ToeplitzLinearOperator
        from linear_operator.utils.interpolation import left_interp, left_t_interp
        from linear_operator.utils.toeplitz import sym_toeplitz_matmul, sym_toeplitz_derivative_quadratic_form
        print("ok")
    """) % os.path.dirname(HERE)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_utils_public_functions():
    from linear_operator_amd.utils.interpolation import left_interp, left_t_interp
    from linear_operator_amd.utils.toeplitz import sym_toeplitz, sym_toeplitz_matmul, toeplitz

    c = T(X["tz_col"][0])
    assert torch.equal(sym_toeplitz(c), toeplitz(c, c))
    v = T(X["tz_rhs"][0])
    assert torch.allclose(sym_toeplitz_matmul(c, v), sym_toeplitz(c) @ v, rtol=1e-4, atol=1e-5)
    li, lv = T(X["sq4_li"][0]), T(X["sq4_lv"][0])
    W = torch.zeros(100, 64).scatter_add_(-1, li, lv)
    u = torch.randn(64, 3)
    assert torch.allclose(left_interp(li, lv, u), W @ u, rtol=1e-5, atol=1e-6)
    w = torch.randn(100, 3)
    assert torch.allclose(left_t_interp(li, lv, w, 64), W.T @ w, rtol=1e-5, atol=1e-5)


def test_pivoted_cholesky_generic_path_unchanged():
    """An existing class (dense) through the generic path: _approx_diagonal is _diagonal there."""
    from linear_operator_amd.operators._linear_operator import LinearOperator

    K = DenseLinearOperator(torch.eye(5))
    assert type(K)._approx_diagonal is LinearOperator._approx_diagonal
    assert torch.equal(K._approx_diagonal(), K._diagonal())
