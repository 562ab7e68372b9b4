"""SKI / Toeplitz on the MI355X: the LO_OP_SKI_DIAG / LO_OP_TOEPLITZ_DIAG kinds and the standalone entry points of
csrc/lo_ski.hip against fp64 numpy and the reference's goldens (tests/golden/g29_ski_*.npz)."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import column, interp, ski_inputs  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.functions import _pivoted_cholesky as _pc  # noqa: E402,F401
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
    KroneckerProductLinearOperator, ToeplitzLinearOperator)

pytestmark = pytest.mark.gpu
X = ski_inputs()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def close(a, b, rel=3e-3):
    a, b = host(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * np.abs(b).max()


def tmv64(t, u):
    """T u in fp64 by circulant embedding (numpy FFT): t [B, M], u [B, M, c] -- no M x M matrix."""
    M = t.shape[-1]
    circ = np.concatenate((t, t[..., 1:][..., ::-1]), -1).astype(np.float64)  # [B, 2M - 1]
    pad = np.zeros((u.shape[0], 2 * M - 1, u.shape[-1]))
    pad[:, :M] = u
    out = np.fft.ifft(np.fft.fft(pad, axis=1) * np.fft.fft(circ, axis=-1)[..., None], axis=1).real
    return out[:, :M]


def wmv64(idx, vals, u):
    """W u in fp64 from the sparse form: idx / vals [B, N, J], u [B, M, c] -> [B, N, c]."""
    g = u.astype(np.float64)[np.arange(idx.shape[0])[:, None, None], idx]  # [B, N, J, c]
    return (g * vals.astype(np.float64)[..., None]).sum(-2)


def wtmv64(idx, vals, v, M):
    """W^T v in fp64 from the sparse form (np.add.at): -> [B, M, c]."""
    B, N, J = idx.shape
    out = np.zeros((B, M, v.shape[-1]))
    contrib = vals.astype(np.float64)[..., None] * v.astype(np.float64)[:, :, None, :]  # [B, N, J, c]
    for b in range(B):
        np.add.at(out[b], idx[b].reshape(-1), contrib[b].reshape(N * J, -1))
    return out


def col_err(y, ref):
    y = np.asarray(y, np.float64)
    return (np.linalg.norm(y - ref, axis=-2) / np.linalg.norm(ref, axis=-2)).max()


@pytest.mark.parametrize("B,M,N,J", [(1, 37, 50, 4), (3, 2048, 3000, 4), (1, 2048, 1500, 16), (1, 16384, 4000, 4)])
@pytest.mark.parametrize("c", [1, 2, 17, 33])
def test_matvec_kinds_and_entry_points(B, M, N, J, c):
    t = column(3000 + M, B, M, ls=0.05)
    li, lv = interp(3001 + M, B, N, M, J)
    ri, rv = interp(3002 + M, B, N, M, J)
    v = np.random.default_rng(M + c).standard_normal((B, N, c)).astype(np.float32)
    d = (0.1 + np.random.default_rng(c).random((B, N))).astype(np.float32)
    for shared in (True, False):
        r_i, r_v = (li, lv) if shared else (ri, rv)
        ref = wmv64(li, lv, tmv64(t, wtmv64(r_i, r_v, v, M))) + d[..., None] * v
        desc = K.ski_diag_descriptor(dev(t), dev(li), dev(lv), dev(r_i), dev(r_v), dev(d))
        assert col_err(host(K.matvec(desc, dev(v))), ref) <= 2e-5
        # the same with the grid-major copy of W_r kept by the caller
        desc.interp_plan = K.interp_plan_build(dev(r_i), M)
        assert col_err(host(K.matvec(desc, dev(v))), ref) <= 2e-5
    u = np.random.default_rng(M).standard_normal((B, M, c)).astype(np.float32)
    assert col_err(host(K.toeplitz_mv(dev(t), dev(u))), tmv64(t, u)) <= 2e-5
    assert col_err(host(K.interp(dev(li), dev(lv), dev(u))), wmv64(li, lv, u)) <= 2e-5
    wtv = wtmv64(li, lv, v, M)
    assert col_err(host(K.interp_t(dev(li), dev(lv), dev(v), M)), wtv) <= 2e-5
    assert col_err(host(K.interp_t_planned(K.interp_plan_build(dev(li), M), dev(lv), dev(v), M)), wtv) <= 2e-5
    # the Toeplitz kind at every grid size, M = 16384 included
    vt = np.random.default_rng(7).standard_normal((B, M, c)).astype(np.float32)
    dt = (0.1 + np.random.default_rng(8).random((B, M))).astype(np.float32)
    y = host(K.matvec(K.toeplitz_diag_descriptor(dev(t), dev(dt)), dev(vt)))
    assert col_err(y, tmv64(t, vt) + dt[..., None] * vt) <= 2e-5


def test_backward_kernels_against_fp64():
    B, M, N, J, S = 2, 300, 500, 4, 5
    rng = np.random.default_rng(11)
    u, v = rng.standard_normal((2, B, M, S)).astype(np.float32)
    g = host(K.toeplitz_bilinear(dev(u), dev(v)))
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    ref = np.zeros((B, M))
    ref[:, 0] = (u64 * v64).sum((1, 2))
    for k in range(1, M):
        ref[:, k] = (u64[:, :-k] * v64[:, k:]).sum((1, 2)) + (u64[:, k:] * v64[:, :-k]).sum((1, 2))
    assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max() * 10
    idx, _ = interp(12, B, N, M, J)
    lvec = rng.standard_normal((B, N, S)).astype(np.float32)
    R = rng.standard_normal((B, M, S)).astype(np.float32)
    gv = host(K.interp_values_grad(dev(idx), dev(lvec), dev(R)))
    refv = np.einsum("bns,bnjs->bnj", lvec.astype(np.float64), R.astype(np.float64)[np.arange(B)[:, None, None], idx])
    assert np.abs(gv - refv).max() <= 1e-5 * np.abs(refv).max()


def test_goldens_forward_and_native_path():
    g = golden("g29_ski_interp")
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(dev(X["sq4_col"])), dev(X["sq4_li"]), dev(X["sq4_lv"]),
                                   dev(X["sq4_ri"]), dev(X["sq4_rv"]))
    K._hip.prof_enable(True)
    y = A._matmul(dev(X["sq4_rhs"]))
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert {"ski_interp", "ski_interp_t", "ski_toeplitz_mv"} <= set(prof), prof.keys()
    assert np.allclose(host(y), g["sq4_matmul"], rtol=1e-4, atol=1e-5)
    for J in (4, 16):
        p = f"sq{J}"
        A = InterpolatedLinearOperator(ToeplitzLinearOperator(dev(X[p + "_col"])), dev(X[p + "_li"]),
                                       dev(X[p + "_lv"]), dev(X[p + "_ri"]), dev(X[p + "_rv"]))
        assert np.allclose(host(A._matmul(dev(X[p + "_rhs"]))), g[p + "_matmul"], rtol=1e-4, atol=1e-5)
        assert np.allclose(host(A._t_matmul(dev(X[p + "_rhs"]))), g[p + "_tmatmul"], rtol=1e-4, atol=1e-5)
        assert np.allclose(host(A.matmul(dev(X[p + "_rhs"]))), g[p + "_mm"], rtol=1e-4, atol=1e-5)
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(dev(X["re_col"])), dev(X["re_li"]), dev(X["re_lv"]),
                                   dev(X["re_ri"]), dev(X["re_rv"]))
    assert np.allclose(host(A.matmul(dev(X["re_rhs"]))), g["re_mm"], rtol=1e-4, atol=1e-5)
    assert np.allclose(host(A._t_matmul(dev(X["re_lhs"]))), g["re_tmatmul"], rtol=1e-4, atol=1e-5)
    bil = A._bilinear_derivative(dev(X["re_lhs"]), dev(X["re_rhs"]))
    assert close(bil[0], g["re_bil_col"], 1e-4) and close(bil[2], g["re_bil_lv"], 1e-4)
    assert close(bil[4], g["re_bil_rv"], 1e-4)
    gt = golden("g29_ski_toeplitz")
    tz = ToeplitzLinearOperator(dev(X["tz_col"]))
    assert np.allclose(host(tz._matmul(dev(X["tz_rhs"]))), gt["tz_matmul"], rtol=1e-4, atol=1e-5)
    assert close(tz._bilinear_derivative(dev(X["tz_u"]), dev(X["tz_v"]))[0], gt["tz_bil"], 1e-4)


def _big(grad=False):
    col, dd, lv = dev(X["big_col"]), dev(X["big_d"]), dev(X["big_lv"])
    li = dev(X["big_li"])
    if grad:
        col, dd, lvl, lvr = (t.clone().requires_grad_(True) for t in (col, dd, lv, lv))
    else:
        lvl = lvr = lv
    return col, dd, li, lvl, lvr


def _no_closure_paths():
    """Patches that fail the test if an engine takes the closure (LO_OP_CALLBACK) path or the generic pivoted Cholesky
    instead of the SKI / Toeplitz descriptor."""
    def boom(*a, **k):
        raise AssertionError("the closure path ran instead of the SKI / Toeplitz kind")

    return (mock.patch.object(K, "_wrap_closure", side_effect=boom),
            mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom))


def test_engines_run_the_new_kinds():
    col, dd, li, lv, _ = _big()
    rhs = dev(X["big_rhs"])
    p1, p2 = _no_closure_paths()
    with p1, p2, settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        for base in (InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv),
                     ToeplitzLinearOperator(dev(column(3300, 2, 2048, ls=0.05)))):
            A = AddedDiagLinearOperator(base, DiagLinearOperator(dd))
            kind = A._kernel_descriptor().kind
            assert kind in (K._hip.LO_OP_SKI_DIAG, K._hip.LO_OP_TOEPLITZ_DIAG)
            K._hip.prof_enable(True)
            x = A.solve(rhs)  # pivoted Cholesky (descriptor rows), preconditioner, CG
            R = A.root_decomposition(method="lanczos").root.to_dense()  # Lanczos
            torch.cuda.synchronize()
            prof = K._hip.prof_report()
            K._hip.prof_enable(False)
            assert "ski_toeplitz_mv" in prof and "pc_update" in prof, prof.keys()
            assert torch.isfinite(x).all() and torch.isfinite(R).all()


def test_pivoted_cholesky_and_determinism():
    g = golden("g29_ski_pivchol")
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(dev(X["pc_col"])), dev(X["pc_li"]), dev(X["pc_lv"]),
                                   dev(X["pc_li"]), dev(X["pc_lv"]))
    assert A._kernel_descriptor() is not None
    from linear_operator_amd.functions import pivoted_cholesky

    L, piv = pivoted_cholesky(A, 10, error_tol=1e-6, return_pivots=True)
    assert np.array_equal(host(piv), g["pc_piv"])
    assert np.abs(host(L) - g["pc_L"]).max() <= 1e-5 * max(1.0, np.abs(g["pc_L"]).max())
    L2, piv2 = pivoted_cholesky(A, 10, error_tol=1e-6, return_pivots=True)
    assert np.array_equal(host(piv2), host(piv)) and np.array_equal(host(L2), host(L))
    col, dd, li, lv, _ = _big()
    desc = K.ski_diag_descriptor(col, li, lv, li, lv, dd)
    v = dev(X["big_rhs"])
    assert np.array_equal(host(K.matvec(desc, v)), host(K.matvec(desc, v)))
    rr = [host(K.interp_t(li, lv, v, 256)) for _ in range(2)]
    assert np.array_equal(rr[0], rr[1])
    A = AddedDiagLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv),
                                DiagLinearOperator(dd))
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        x1, x2 = host(A.solve(v)), host(A.solve(v))
    assert np.array_equal(x1, x2)


def test_solves_and_gradients_against_golden():
    g = golden("g29_ski_solve")
    Z = dev(X["big_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    col, dd, li, lv, _ = _big()
    rhs = dev(X["big_rhs"])
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        A = AddedDiagLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv),
                                    DiagLinearOperator(dd))
        assert A._kernel_descriptor().kind == K._hip.LO_OP_SKI_DIAG
        x = A.solve(rhs)
        assert np.allclose(host(x), g["big_solve"], rtol=1e-4, atol=1e-4 * np.abs(g["big_solve"]).max())
        colg, ddg, li, lvl, lvr = _big(grad=True)
        A = Probed(InterpolatedLinearOperator(ToeplitzLinearOperator(colg), li, lvl, li, lvr), DiagLinearOperator(ddg))
        iq, ld = A.inv_quad_logdet(rhs, logdet=True)
        assert np.allclose(host(iq), g["big_iq"], rtol=1e-4, atol=0)
        assert np.allclose(host(ld), g["big_ld"], rtol=1e-4, atol=2048 * 1.2e-7 * 10.0)
        (iq.sum() + ld.sum()).backward()
    assert close(colg.grad, g["big_dcol"]) and close(ddg.grad, g["big_dd"])
    assert close(lvl.grad, g["big_dlv"]) and close(lvr.grad, g["big_drv"])


def test_lanczos_root_and_samples():
    col, dd, li, lv, _ = _big()
    A = AddedDiagLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv),
                                DiagLinearOperator(dd))
    R = A.root_decomposition(method="lanczos").root.to_dense()
    k = R.shape[-1]
    assert R.shape[:-1] == (2, 2048) and 1 <= k
    # R R^T agrees with A on the Krylov space: the columns of R span it
    q = torch.linalg.qr(R)[0]
    assert close(R @ (R.mT @ q), host(A._matmul(q.contiguous())), 1e-3)
    ski = InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv)
    s = ski.zero_mean_mvn_samples(3)
    assert s.shape == (3, 2, 2048) and torch.isfinite(s).all()


def test_large_grid_fallback_and_2d_forward():
    M, N = 20000, 500
    t = column(3100, 1, M, ls=0.01)
    li, lv = interp(3101, 1, N, M, 4)
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(dev(t)), dev(li), dev(lv), dev(li), dev(lv))
    assert A._kernel_descriptor() is None  # beyond LO_TOEPLITZ_MAX_M: the torch composition
    v = np.random.default_rng(1).standard_normal((1, N, 2)).astype(np.float32)
    ref = wmv64(li, lv, tmv64(t, wtmv64(li, lv, v, M)))
    assert col_err(host(A._matmul(dev(v))), ref) <= 1e-4
    g = golden("g29_ski_kron2d")
    base = KroneckerProductLinearOperator(ToeplitzLinearOperator(dev(X["k2_c1"])),
                                          ToeplitzLinearOperator(dev(X["k2_c2"])))
    A2 = InterpolatedLinearOperator(base, dev(X["k2_li"]), dev(X["k2_lv"]), dev(X["k2_li"]), dev(X["k2_lv"]))
    assert np.allclose(host(A2._matmul(dev(X["k2_rhs"]))), g["k2_matmul"], rtol=1e-4, atol=1e-5)
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        x = AddedDiagLinearOperator(A2, DiagLinearOperator(dev(X["k2_d"]))).solve(dev(X["k2_rhs"]))
    assert np.allclose(host(x), g["k2_solve"], rtol=1e-3, atol=1e-3 * np.abs(g["k2_solve"]).max())
    c1 = dev(X["k2_c1"]).requires_grad_(True)
    base = KroneckerProductLinearOperator(ToeplitzLinearOperator(c1), ToeplitzLinearOperator(dev(X["k2_c2"])))
    A2 = InterpolatedLinearOperator(base, dev(X["k2_li"]), dev(X["k2_lv"]), dev(X["k2_li"]), dev(X["k2_lv"]))
    with pytest.raises(NotImplementedError):
        (A2.matmul(dev(X["k2_rhs"]))).sum().backward()


def test_gpytorch_scale_preconditioned_cg():
    """S2 of tools/mb_ski.py with cubic weights: a preconditioned CG solve reaches the tolerance; residual in fp64."""
    B, N, M, J = 64, 16384, 2048, 4
    t = column(3200, B, M, ls=0.02)
    li, lv = interp(3201, B, N, M, J, cubic=True)
    rhs = np.random.default_rng(3202).standard_normal((B, N, 1)).astype(np.float32)
    A = AddedDiagLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(dev(t)), dev(li), dev(lv),
                                                           dev(li), dev(lv)),
                                ConstantDiagLinearOperator(torch.full((B, 1), 0.01, device="cuda"), N))
    with settings.cg_tolerance(1e-4), settings.max_cg_iterations(1000):
        x = host(A.solve(dev(rhs))).astype(np.float64)
        # the same solve through the engine directly, to see that CG CONVERGED: below the iteration cap, with the
        # reference's stopping rule (mean relative recursive residual < tolerance, linear_cg.py) satisfied
        closure = A._preconditioner()[0]
        res = K.cg_solve(A._kernel_descriptor(), dev(rhs), precond=closure.woodbury, tolerance=1e-4, max_iter=1000)
    assert res.tolerance_reached and res.iterations < 1000 and res.mean_residual < 1e-4, (res.iterations,
                                                                                           res.mean_residual)
    assert np.allclose(host(res.x), x, rtol=1e-3, atol=1e-3 * np.abs(x).max())
    true_res = []
    for b in range(0, B, 16):
        Ax = wmv64(li[b:b + 1], lv[b:b + 1], tmv64(t[b:b + 1], wtmv64(li[b:b + 1], lv[b:b + 1], x[b:b + 1], M)))
        Ax = Ax[0] + 0.01 * x[b]
        true_res.append(np.linalg.norm(Ax - rhs[b]) / np.linalg.norm(rhs[b]))
    # (the true residual of the fp32 iterate, evaluated in fp64, lies above the recursive one: the fp32 floor of this
    # conditioning, a few 1e-3; convergence itself is asserted above)
    assert max(true_res) < 1e-2, true_res
