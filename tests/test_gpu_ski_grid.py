"""SKI on a 2-D / 3-D grid on the MI355X: the grid product of csrc/lo_ski_grid.hip against the fp64 dense Kronecker
product, the LO_OP_SKI_GRID_DIAG kind through lo_matvec_f32, `_matmul`, CG, Lanczos and the pivoted Cholesky against the
reference's goldens (tests/golden/g35_ski_grid.npz)."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import column, rng  # noqa: E402
from make_golden_ski_grid import PC_RANK, grid_inputs, grid_interp, kron_dense64, w_dense64  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.functions import pivoted_cholesky  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
    KroneckerProductLinearOperator, ToeplitzLinearOperator)

pytestmark = pytest.mark.gpu
X = grid_inputs()
G = np.load(os.path.join(HERE, "golden", "g35_ski_grid.npz"))
C2, C3 = ("g2_c1", "g2_c2"), ("g3_c1", "g3_c2", "g3_c3")
CASES = [(C2, "g2b1", False), (C2, "g2b3", False), (C3, "g3", False), (C2, "lr", True)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def close(a, b, rel=3e-3):
    a, b = host(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * np.abs(b).max()


def col_err(y, ref):
    y = np.asarray(y, np.float64)
    return (np.linalg.norm(y - ref, axis=-2) / np.linalg.norm(ref, axis=-2)).max()


def kron_apply64(cols, u):
    """(T_1 (x) .. (x) T_D) u in fp64 for one member: the dense symmetric Toeplitz matrix of every factor applied along
    its axis of u [M_1, .., M_D, c] (the Kronecker product itself is not formed: 8450^2 entries at the largest shape)."""
    y = u.astype(np.float64).reshape(*[t.shape[-1] for t in cols], -1)
    for k, t in enumerate(cols):
        m = t.shape[-1]
        Tk = t.astype(np.float64)[np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])]
        y = np.moveaxis(np.tensordot(Tk, y, axes=(1, k)), 0, k)
    return y.reshape(u.shape)


def operator(cols, p, separate=False, lv=None, rv=None):
    base = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(dev(X[c])) for c in cols])
    li = dev(X[p + "_li"])
    lv = dev(X[p + "_lv"]) if lv is None else lv
    if separate:
        return InterpolatedLinearOperator(base, li, lv, dev(X[p + "_ri"]), dev(X[p + "_rv"]))
    return InterpolatedLinearOperator(base, li, lv, li, lv if rv is None else rv)


@pytest.mark.parametrize("grid,c,B", [((5, 7), 1, 1), ((1, 8), 2, 1), ((33, 20), 3, 1), ((130, 65), 17, 2),
                                      ((6, 5, 4), 2, 1), ((17, 9, 33), 5, 1), ((1024, 3), 1, 1),
                                      ((96, 64), 24, 8)])  # (the last: enough workgroups for 8 rows per thread)
def test_grid_product_against_fp64_dense_kronecker(grid, c, B):
    cols = [column(3600 + k, B, m, ls=0.2) * (1.0 + 0.1 * rng(3610 + k).standard_normal((B, m))).astype(np.float32)
            for k, m in enumerate(grid)]
    M = int(np.prod(grid))
    u = rng(3620 + M).standard_normal((B, M, c)).astype(np.float32)
    y = host(K.toeplitz_kron_mv([dev(t) for t in cols], dev(u)))
    ref = np.stack([kron_apply64([t[b] for t in cols], u[b]) for b in range(B)])
    assert col_err(y, ref) <= 1e-4


@pytest.mark.parametrize("grid", [(1025, 2), (64,), (4, 4, 4, 4)])
def test_grid_product_refuses_what_it_does_not_take(grid):
    cols = [dev(column(3630 + k, 1, m)) for k, m in enumerate(grid)]
    u = torch.zeros(1, int(np.prod(grid)), 1, device="cuda")
    with pytest.raises(K._hip.HipExtensionError, match="unsupported"):
        K.toeplitz_kron_mv(cols, u)


@pytest.mark.parametrize("cols,p,separate", CASES)
def test_kind_through_matvec_and_matmul_against_goldens(cols, p, separate):
    A = operator(cols, p, separate)
    desc = A._kernel_descriptor()
    assert desc.kind == K._hip.LO_OP_SKI_GRID_DIAG and desc.grid == tuple(X[c].shape[-1] for c in cols)
    for c in (1, 5):
        rhs = dev(X[f"{p}_rhs{c}"])
        assert np.allclose(host(K.matvec(desc, rhs)), G[f"{p}_mm{c}"], rtol=1e-4, atol=1e-5)
        assert np.allclose(host(A._matmul(rhs)), G[f"{p}_mm{c}"], rtol=1e-4, atol=1e-5)


def test_out_of_range_indices_contribute_nothing():
    cols = [X[c] for c in C2]
    M = 12 * 16
    li, lv, ri, rv = (X[k].copy() for k in ("lr_li", "lr_lv", "lr_ri", "lr_rv"))
    li[0, 3, 2], li[0, 100, 0], ri[0, 7, 5], ri[0, 150, 15] = M, -1, -1, M
    desc = K.ski_grid_diag_descriptor([dev(t[None]) for t in cols], dev(li), dev(lv), dev(ri), dev(rv), None)
    assert desc.kind == K._hip.LO_OP_SKI_GRID_DIAG
    y = host(K.matvec(desc, dev(X["lr_rhs5"])))
    lz, rz = lv.copy(), rv.copy()
    lz[0, 3, 2] = lz[0, 100, 0] = rz[0, 7, 5] = rz[0, 150, 15] = 0.0
    Wl = w_dense64(np.clip(li[0], 0, M - 1), lz[0], M)
    Wr = w_dense64(np.clip(ri[0], 0, M - 1), rz[0], M)
    ref = Wl @ (kron_dense64(cols) @ (Wr.T @ X["lr_rhs5"][0].astype(np.float64)))
    assert col_err(y[0], ref) <= 1e-4


def test_descriptor_routing():
    for cols, p, separate in CASES:
        assert operator(cols, p, separate)._kernel_descriptor().kind == K._hip.LO_OP_SKI_GRID_DIAG
    li, lv = dev(X["g2b1_li"]), dev(X["g2b1_lv"])
    tz = lambda k, dtype=torch.float32, device="cuda": ToeplitzLinearOperator(  # noqa: E731
        torch.from_numpy(X[k]).to(device=device, dtype=dtype))
    kron = KroneckerProductLinearOperator
    assert InterpolatedLinearOperator(kron(tz("g2_c1", torch.float64), tz("g2_c2", torch.float64)), li,
                                      lv.double(), li, lv.double())._kernel_descriptor() is None
    assert InterpolatedLinearOperator(kron(tz("g2_c1", device="cpu"), tz("g2_c2", device="cpu")), li.cpu(), lv.cpu(),
                                      li.cpu(), lv.cpu())._kernel_descriptor() is None
    four = kron(*[ToeplitzLinearOperator(dev(column(3640 + k, 1, 4)[0])) for k in range(4)])
    i4, v4 = grid_interp(3645, 1, 40, (4, 4, 4, 4), pts=2)
    assert InterpolatedLinearOperator(four, dev(i4), dev(v4), dev(i4), dev(v4))._kernel_descriptor() is None
    dense = kron(tz("g2_c1"), DenseLinearOperator(tz("g2_c2").to_dense()))
    assert InterpolatedLinearOperator(dense, li, lv, li, lv)._kernel_descriptor() is None
    assert InterpolatedLinearOperator(kron(tz("g2_c1"), tz("g2_c2")), li[:, :100], lv[:, :100], li,
                                      lv)._kernel_descriptor() is None  # rectangular
    wide = kron(ToeplitzLinearOperator(dev(column(3650, 1, 1025)[0])), ToeplitzLinearOperator(dev(column(3651, 1, 4)[0])))
    iw, vw = grid_interp(3652, 1, 50, (1025, 4))
    assert InterpolatedLinearOperator(wide, dev(iw), dev(vw), dev(iw), dev(vw))._kernel_descriptor() is None


def _no_closure_paths():
    """Patches that fail the test if an engine takes the closure (LO_OP_CALLBACK) path or the generic pivoted Cholesky
    instead of the grid descriptor."""
    def boom(*a, **k):
        raise AssertionError("the closure path ran instead of the SKI grid kind")

    return (mock.patch.object(K, "_wrap_closure", side_effect=boom),
            mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom))


def _solver_settings():
    return (settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.max_cholesky_size(0),
            settings.min_preconditioning_size(100))


def test_engines_run_the_grid_kind():
    A = AddedDiagLinearOperator(operator(C2, "g2b1"), DiagLinearOperator(dev(X["g2b1_d"])))
    assert A._kernel_descriptor().kind == K._hip.LO_OP_SKI_GRID_DIAG
    p1, p2 = _no_closure_paths()
    s1, s2, s3, s4 = _solver_settings()
    with p1, p2, s1, s2, s3, s4:
        K._hip.prof_enable(True)
        x = A.solve(dev(X["g2b1_rhs"]))  # pivoted Cholesky (descriptor rows), preconditioner, CG
        R = A.root_decomposition(method="lanczos").root.to_dense()  # Lanczos
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
    assert "ski_grid_mv" in prof and "pc_update" in prof, prof.keys()
    assert torch.isfinite(R).all()
    ref = G["g2b1_solve"]
    assert np.allclose(host(x), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())
    s1, s2, s3, s4 = _solver_settings()
    with s1, s2, s3, s4:
        A3 = AddedDiagLinearOperator(operator(C2, "g2b3"), DiagLinearOperator(dev(X["g2b3_d"])))
        x3 = A3.solve(dev(X["g2b3_rhs"]))
    ref = G["g2b3_solve"]
    assert np.allclose(host(x3), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())


def test_pivoted_cholesky_against_golden():
    A = operator(C2, "pc")
    p1, p2 = _no_closure_paths()
    with p1, p2:
        L, piv = pivoted_cholesky(A, PC_RANK, error_tol=1e-6, return_pivots=True)
    assert np.array_equal(host(piv), G["pc_piv"])
    assert np.abs(host(L) - G["pc_L"]).max() <= 1e-5 * max(1.0, np.abs(G["pc_L"]).max())


def test_determinism():
    A = operator(C3, "g3")
    desc = A._kernel_descriptor()
    v = dev(X["g3_rhs5"])
    assert np.array_equal(host(K.matvec(desc, v)), host(K.matvec(desc, v)))
    P = operator(C2, "pc")
    r = [pivoted_cholesky(P, PC_RANK, error_tol=1e-6, return_pivots=True) for _ in range(2)]
    assert np.array_equal(host(r[0][0]), host(r[1][0])) and np.array_equal(host(r[0][1]), host(r[1][1]))
    S = AddedDiagLinearOperator(operator(C2, "g2b3"), DiagLinearOperator(dev(X["g2b3_d"])))
    s1, s2, s3, s4 = _solver_settings()
    with s1, s2, s3, s4:
        x1, x2 = host(S.solve(dev(X["g2b3_rhs"]))), host(S.solve(dev(X["g2b3_rhs"])))
    assert np.array_equal(x1, x2)


def test_inv_quad_logdet_forward_and_backward_against_golden():
    Z = dev(X["g2b1_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    dd, lvl, lvr = (dev(X[k]).clone().requires_grad_(True) for k in ("g2b1_d", "g2b1_lv", "g2b1_lv"))
    s1, s2, s3, s4 = _solver_settings()
    with s1, s2, s3, s4, settings.num_trace_samples(6):
        A = Probed(operator(C2, "g2b1", lv=lvl, rv=lvr), DiagLinearOperator(dd))
        assert A._kernel_descriptor().kind == K._hip.LO_OP_SKI_GRID_DIAG
        iq, ld = A.inv_quad_logdet(dev(X["g2b1_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
    assert close(iq, G["iql_iq"]) and close(ld, G["iql_ld"])
    assert close(dd.grad, G["iql_dd"]) and close(lvl.grad, G["iql_dlv"]) and close(lvr.grad, G["iql_drv"])
    # gradients with respect to the columns of a Kronecker base stay out of scope
    c1 = dev(X["g2_c1"]).requires_grad_(True)
    base = KroneckerProductLinearOperator(ToeplitzLinearOperator(c1), ToeplitzLinearOperator(dev(X["g2_c2"])))
    li, lv = dev(X["g2b1_li"]), dev(X["g2b1_lv"])
    with pytest.raises(NotImplementedError):
        InterpolatedLinearOperator(base, li, lv, li, lv).matmul(dev(X["g2b1_rhs"])).sum().backward()
