"""GPU parity tests proper: the HIP path (through the C ABI, linear_operator_amd.kernels) against
 (a) the CPU oracle on the same seeded inputs and (b) the golden vectors the real reference produced.
Bars: integer results (pivots / permutations / iteration counts at the floors) bit-exact; fp32 solves
within 1e-4 relative per column (north_star); logdet within 1e-4 rel + the documented eigensolver noise
floor.  Run with `pytest -m gpu` on an MI355X.
"""
import warnings

import numpy as np
import pytest
import torch

import cases
from conftest import load_golden, max_rel_err_cols, rel_err
from oracle import lo_oracle as orc

pytestmark = pytest.mark.gpu

from linear_operator_amd import kernels as K  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _resident_ran(prof):
    """One of the operator-resident CG kernels ran (serial-column generations or the 16-column lockstep kernel)."""
    return "cg_onchip" in prof or "cg_lockstep" in prof


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------- matvecs
@pytest.mark.parametrize("c", [1, 2, 5, 8, 17])
@pytest.mark.parametrize("R", [8, 15, 32])
def test_matvec_lowrank_diag(c, R):
    C, d, v = cases.lowrank_diag(1000 + c + R, 3, 1000, R, c)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    y = host(K.matvec(desc, dev(v)))
    ref = orc.matvec_lowrank_diag(C.astype(np.float64), d.astype(np.float64), v.astype(np.float64))
    assert max_rel_err_cols(y, ref) < 2e-6
    # constant diagonal + no diagonal
    sig = np.array([0.25, 0.5, 2.0], dtype=np.float32)
    y2 = host(K.matvec(K.lowrank_diag_descriptor(dev(C), dev(sig), const_diag=True), dev(v)))
    ref2 = orc.matvec_lowrank_diag(C.astype(np.float64), np.broadcast_to(sig[:, None], d.shape).astype(np.float64),
                                   v.astype(np.float64))
    assert max_rel_err_cols(y2, ref2) < 2e-6
    y3 = host(K.matvec(K.lowrank_diag_descriptor(dev(C), None), dev(v)))
    assert max_rel_err_cols(y3, orc.matvec_lowrank_diag(C.astype(np.float64), 0 * d.astype(np.float64),
                                                        v.astype(np.float64))) < 2e-6


def test_matvec_golden_g6():
    g = load_golden("g6_matmul")
    C, d, v = cases.lowrank_diag(601, 3, 256, 8, 5)
    Kd, dd, vv = cases.dense_diag(611, 2, 96, 3)
    K1, K2, s, vk = cases.kron_factors(621, 2, 12, 20, 3)
    tol = dict(rtol=1e-4, atol=1e-4)
    assert np.allclose(host(K.matvec(K.lowrank_diag_descriptor(dev(C), dev(d)), dev(v))), g["y_lowrank_diag"], **tol)
    assert np.allclose(host(K.matvec(K.lowrank_diag_descriptor(dev(C), None), dev(v))), g["y_lowrank"], **tol)
    assert np.allclose(host(K.matvec(K.dense_diag_descriptor(dev(Kd), dev(dd)), dev(vv))), g["y_dense_diag"], **tol)
    assert np.allclose(host(K.matvec(K.dense_diag_descriptor(dev(Kd), None), dev(vv))), g["y_dense"], **tol)
    assert np.allclose(host(K.matvec(K.kron_diag_descriptor(dev(K1), dev(K2), None), dev(vk))), g["y_kron"], **tol)
    assert np.allclose(host(K.matvec(K.kron_diag_descriptor(dev(K1), dev(K2), dev(s[:, 0]), const_diag=True), dev(vk))),
                       g["y_kron_diag"], **tol)


@pytest.mark.parametrize("c", [1, 3, 6])
def test_matvec_dense_and_kron(c):
    Kd, dd, vv = cases.dense_diag(1100 + c, 2, 520, c)
    y = host(K.matvec(K.dense_diag_descriptor(dev(Kd), dev(dd)), dev(vv)))
    ref = orc.matvec_dense_diag(Kd.astype(np.float64), dd.astype(np.float64), vv.astype(np.float64))
    assert max_rel_err_cols(y, ref) < 5e-6
    K1, K2, s, vk = cases.kron_factors(1200 + c, 3, 24, 40, c)
    y = host(K.matvec(K.kron_diag_descriptor(dev(K1), dev(K2), dev(s[:, 0]), const_diag=True), dev(vk)))
    dk = np.broadcast_to(s, (3, 960)).astype(np.float64)
    ref = orc.matvec_kron_diag(K1.astype(np.float64), K2.astype(np.float64), dk, vk.astype(np.float64))
    assert max_rel_err_cols(y, ref) < 5e-6


@pytest.mark.parametrize("n1,n2", [(128, 256), (256, 128)])
def test_matvec_and_cg_kron_matrix_core_engine(n1, n2):
    """c == 1 and factors that are multiples of 128 take the MFMA engine (intermediate produced transposed, diagonal
    term and CG dot partials fused in the epilogue): product against the fp64 oracle, CG against the VALU engine
    (3 identical columns force it) and the oracle."""
    K1, K2, s, vk = cases.kron_factors(1300 + n1, 3, n1, n2, 1)
    N = n1 * n2
    dfull = cases.randn(1301, 3, N, 1, dtype=np.float32)[..., 0] ** 2 + 0.5
    for desc, dk in ((K.kron_diag_descriptor(dev(K1), dev(K2), dev(s[:, 0]), const_diag=True),
                      np.broadcast_to(s, (3, N)).astype(np.float64)),
                     (K.kron_diag_descriptor(dev(K1), dev(K2), dev(dfull)), dfull.astype(np.float64))):
        K._hip.prof_enable(True)
        y = host(K.matvec(desc, dev(vk)))
        torch.cuda.synchronize()
        assert "kron_gemm_mfma" in K._hip.prof_report()
        K._hip.prof_enable(False)
        ref = orc.matvec_kron_diag(K1.astype(np.float64), K2.astype(np.float64), dk, vk.astype(np.float64))
        assert max_rel_err_cols(y, ref) < 5e-6
    desc = K.kron_diag_descriptor(dev(K1), dev(K2), dev(s[:, 0]), const_diag=True)
    res = K.cg_solve(desc, dev(vk), tolerance=1e-3, max_iter=400)
    res3 = K.cg_solve(desc, dev(np.repeat(vk, 3, axis=-1)), tolerance=1e-3, max_iter=400)  # VALU engine (c = 3)
    assert abs(res.iterations - res3.iterations) <= 1 and res.tolerance_reached
    assert max_rel_err_cols(host(res.x), host(res3.x)[..., :1]) < 2e-3
    dk = np.broadcast_to(s, (3, N)).astype(np.float32)
    xo, _, info = orc.linear_cg(lambda v: orc.matvec_kron_diag(K1, K2, dk, v), vk, tolerance=1e-3, max_iter=400)
    assert abs(info.iterations - res.iterations) <= 1
    assert max_rel_err_cols(host(res.x), xo) < 2e-3


# ------------------------------------------------------------------------------------------- linear_cg
def test_cg_lowrank_no_precond_vs_golden_and_oracle():
    g = load_golden("g1_cg_fp32_lowrank")
    C, d, rhs = cases.lowrank_diag(141, 4, 512, 8, 5)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    res = K.cg_solve(desc, dev(rhs), tolerance=1.0)
    # 11-iteration floor; the reference spends one more product on A @ 0, we skip it
    assert res.iterations == int(g["matvecs_tol1"]) - 1 == 11 and res.tolerance_reached
    assert max_rel_err_cols(host(res.x), g["x_tol1"]) < 1e-4
    res = K.cg_solve(desc, dev(rhs), tolerance=1.0, n_tridiag=4)
    assert res.iterations == int(g["matvecs_t_tol1"]) - 1 == 21
    assert res.t_mat.shape == g["t_mat_tol1"].shape
    assert max_rel_err_cols(host(res.x), g["xt_tol1"]) < 1e-4
    assert rel_err(host(res.t_mat)[..., :8, :8], g["t_mat_tol1"][..., :8, :8]) < 1e-3
    res = K.cg_solve(desc, dev(rhs), tolerance=1e-4)
    assert abs(res.iterations - (int(g["matvecs_tol1e4"]) - 1)) <= 1  # fp32 noise regime, see oracle test
    assert max_rel_err_cols(host(res.x), g["x_tol1e4"]) < 1e-4
    # zero column + initial guess: one CG step from x0 then frozen
    rhs_z = rhs.copy()
    rhs_z[1, :, 2] = 0.0
    x0 = cases.randn(142, 4, 512, 5, dtype=np.float32) * 0.1
    res = K.cg_solve(desc, dev(rhs_z), x0=dev(x0), tolerance=1e-4)
    assert res.matvecs == int(g["matvecs_zero_col"]) or abs(res.matvecs - int(g["matvecs_zero_col"])) <= 1
    assert np.allclose(host(res.x)[1, :, 2], g["x_zero_col"][1, :, 2], rtol=1e-4, atol=1e-6)
    assert max_rel_err_cols(np.delete(host(res.x), 2, -1), np.delete(g["x_zero_col"], 2, -1)) < 1e-4
    res = K.cg_solve(desc, dev(rhs_z), tolerance=1e-4)
    assert np.all(host(res.x)[1, :, 2] == 0)


def test_cg_fp32_reference_recipe_dense_callback_and_native():
    """test_linear_cg.py:27-64 recipe in fp32 (kernels are fp32): CG vs direct solve, atol 1e-3 / rtol 1e-4."""
    M = cases.spd_test_matrix(101, 100, dtype=np.float32)
    b = cases.randn(103, 100, 50, dtype=np.float32)
    actual = np.linalg.solve(M.astype(np.float64), b.astype(np.float64))
    Mt = dev(M)
    res = K.cg_solve(None, dev(b), matvec_closure=lambda v: Mt @ v, max_iter=100, tolerance=1e-6)
    assert np.allclose(host(res.x), actual, atol=1e-3, rtol=1e-4)
    desc = K.dense_diag_descriptor(dev(M[None]), None)
    res2 = K.cg_solve(desc, dev(b[None]), max_iter=100, tolerance=1e-6)
    assert np.allclose(host(res2.x)[0], actual, atol=1e-3, rtol=1e-4)
    # same algorithm through both paths
    assert res.iterations == res2.iterations or abs(res.iterations - res2.iterations) <= 2
    xo, _, info = orc.linear_cg(lambda v: M @ v, b, max_iter=100, tolerance=1e-6)
    assert abs(info.iterations - res2.iterations) <= 2


def test_cg_tridiag_eigenvalues_small():
    """test_linear_cg.py:66-95: tridiagonals of a 10x10 system reproduce its spectrum."""
    M = cases.spd_test_matrix(111, 10, dtype=np.float32)
    b = cases.randn(112, 10, 50, dtype=np.float32)
    res = K.cg_solve(K.dense_diag_descriptor(dev(M[None]), None), dev(b[None]), n_tridiag=5, max_tridiag_iter=10,
                     max_iter=10, tolerance=0.0, eps=1e-15)
    assert not res.tolerance_reached and res.iterations == 10  # -> NumericalWarning in the shim
    eigs = np.linalg.eigvalsh(M.astype(np.float64))
    t = host(res.t_mat)
    assert t.shape == (5, 1, 10, 10)
    for i in range(5):
        assert np.allclose(eigs, np.linalg.eigvalsh(t[i, 0].astype(np.float64)), atol=1e-3, rtol=1e-3)


def test_cg_nan_detection_and_skip():
    C, d, rhs = cases.lowrank_diag(77, 2, 300, 8, 2)
    Cn = C.copy()
    Cn[0, 5, 1] = np.nan
    res = K.cg_solve(K.lowrank_diag_descriptor(dev(Cn), dev(d)), dev(rhs))
    assert res.nan_detected
    res = K.cg_solve(K.lowrank_diag_descriptor(dev(Cn), dev(d)), dev(rhs), x0=dev(rhs * 0.1))
    assert res.nan_detected
    res = K.cg_solve(K.lowrank_diag_descriptor(dev(C), dev(d)), dev(np.zeros_like(rhs)))
    assert res.skipped and res.iterations == 0 and np.all(host(res.x) == 0)


# ------------------------------------------------------------------------------------------- pivoted Cholesky
def _check_pivchol(desc, src, rank, golden_L=None, golden_piv=None):
    L, piv = K.pivoted_cholesky(desc, rank)
    Lo, pivo = orc.pivoted_cholesky(src, rank)
    assert np.array_equal(host(piv), pivo), "pivots / permutation must be bit-exact"
    assert host(L).shape == Lo.shape
    assert np.array_equal(host(L), Lo), "same operation order -> L must be bit-identical to the oracle"
    if golden_piv is not None:
        assert np.array_equal(host(piv), golden_piv)
        assert np.allclose(host(L), golden_L, rtol=1e-4, atol=1e-5)


def test_pivoted_cholesky_bit_exact():
    g = load_golden("g2_pivchol_lowrank")
    for R in (8, 32):
        C = cases.lowrank_diag(210 + R, 3, 2048, R, 1)[0]
        _check_pivchol(K.lowrank_diag_descriptor(dev(C), None), orc.LowRankRowSource(C), 15, g[f"L_R{R}"],
                       g[f"piv_R{R}"])
    g = load_golden("g2_pivchol_kron_dense")
    K1, K2, _, _ = cases.kron_factors(221, 2, 16, 16, 1)
    _check_pivchol(K.kron_diag_descriptor(dev(K1), dev(K2), None), orc.KronRowSource(K1, K2), 15, g["L_kron"],
                   g["piv_kron"])
    Kd = cases.dense_diag(222, 2, 300, 1)[0]
    _check_pivchol(K.dense_diag_descriptor(dev(Kd), None), orc.DenseRowSource(Kd), 15, g["L_dense"], g["piv_dense"])
    g = load_golden("g2_pivchol_dense8")
    m8 = cases.pivchol_dense8(201)
    _check_pivchol(K.dense_diag_descriptor(dev(m8[None]), None), orc.DenseRowSource(m8[None]), 3, g["L"][None],
                   g["piv"][None])
    mb = cases.pivchol_dense8(202, batch=(2, 3))
    L, piv = K.pivoted_cholesky(K.dense_diag_descriptor(dev(mb), None), 3)
    assert tuple(L.shape) == (2, 3, 8, 3) and np.array_equal(host(piv), g["pivb"])
    assert np.allclose(host(L), g["Lb"], rtol=1e-5, atol=1e-6)
    L8, piv8 = K.pivoted_cholesky(K.dense_diag_descriptor(dev(m8[None]), None), 8)  # rank == N edge
    assert np.array_equal(host(piv8)[0], g["piv8"]) and tuple(L8.shape) == (1, 8, g["L8"].shape[-1])


def test_pivoted_cholesky_bench_shape_bit_exact():
    """cfg2-shaped (N=8192, R=32), more members: pivots and L bit-identical to the oracle."""
    C = cases.lowrank_diag(2301, 6, 8192, 32, 1)[0]
    _check_pivchol(K.lowrank_diag_descriptor(dev(C), None), orc.LowRankRowSource(C), 15)


@pytest.mark.parametrize("N,R,B", [(8192, 32, 70), (4096, 16, 33), (1500, 8, 5), (5000, 32, 9), (12000, 16, 3),
                                   (4096, 20, 7), (3000, 5, 4), (8192, 30, 10),  # (ranks padded to 8 / 16 / 32)
                                   (20000, 32, 5), (32768, 16, 4)])  # (groups of 32 workgroups)
def test_onchip_pivoted_cholesky_matches_streaming_engine_and_oracle(N, R, B):
    """Operator-resident pivoted Cholesky (one 8-workgroup group per member, C rows in LDS, L rows in VGPRs, one
    granule exchange per pivot): L, permutation and rank bit-identical to the streaming engine and to the oracle."""
    C = cases.lowrank_diag(3300 + R, B, N, R, 1)[0]
    desc = K.lowrank_diag_descriptor(dev(C), None)
    try:
        K.set_onchip_cg(False)
        Ls, ps = K.pivoted_cholesky(desc, 15)
        K.set_onchip_cg(True)
        K._hip.prof_enable(True)
        Lo, po = K.pivoted_cholesky(desc, 15)
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
    finally:
        K.set_onchip_cg(True)
    assert "pc_onchip" in prof, "fast path was not taken"
    assert Lo.shape == Ls.shape
    assert torch.equal(po, ps) and torch.equal(Lo, Ls)
    sub = slice(0, 3)
    Lr, pr = orc.pivoted_cholesky(orc.LowRankRowSource(C[sub]), 15)
    assert np.array_equal(host(po)[sub], pr) and np.array_equal(host(Lo)[sub], Lr)
    # early stop through the batch-global tolerance rule (_pivoted_cholesky.py:57): same m, same permutation
    for tol in (0.5, 0.9):
        try:
            K.set_onchip_cg(False)
            Ls, ps = K.pivoted_cholesky(desc, 15, error_tol=tol)
        finally:
            K.set_onchip_cg(True)
        Lo, po = K.pivoted_cholesky(desc, 15, error_tol=tol)
        assert Lo.shape == Ls.shape and torch.equal(po, ps) and torch.equal(Lo, Ls)
    if R <= 8:  # rank-deficient root: the error collapses after R pivots and the loop stops on its own
        Lo, po = K.pivoted_cholesky(desc, 15, error_tol=1e-3)
        assert Lo.shape[-1] < 15


# ------------------------------------------------------------------------------------------- preconditioner
def test_preconditioner_build_apply():
    g = load_golden("g3_precond")
    C, d, rhs = cases.lowrank_diag(301, 3, 2048, 32, 4)
    L, _ = K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C), None), 15)
    assert np.allclose(host(L), g["L_nonconst"], rtol=1e-4, atol=1e-5)
    pre = K.precond_build(L, dev(d), constant_diag=False)
    z = host(K.precond_apply(pre, dev(rhs)))
    assert max_rel_err_cols(z, g["z_nonconst"]) < 1e-5
    assert np.allclose(host(pre.logdet), g["logdet_nonconst"], rtol=1e-5)
    sig = np.array([0.3, 0.7, 1.1], dtype=np.float32)
    pre = K.precond_build(L, dev(sig), constant_diag=True)
    z = host(K.precond_apply(pre, dev(rhs)))
    assert max_rel_err_cols(z, g["z_const"]) < 1e-5
    assert np.allclose(host(pre.logdet), g["logdet_const"], rtol=1e-5, atol=1e-2)
    # against the oracle in fp64
    po = orc.Preconditioner(host(L).astype(np.float64), np.broadcast_to(sig[:, None], (3, 2048)).astype(np.float64))
    assert max_rel_err_cols(z, po.apply(rhs.astype(np.float64))) < 1e-5


# ------------------------------------------------------------------------------------------- solve / inv_quad_logdet
def _default_precond(desc, d_t, const, root_form=True):
    """Rank-15 pivoted-Cholesky preconditioner.  For low-rank operators also in ROOT FORM (what the resident kernels
    prefer); the generic Q form is always built as well (the streaming engine and precond_apply use it)."""
    L, perm = K.pivoted_cholesky(desc, 15)
    if root_form and desc.kind == K._hip.LO_OP_LOWRANK_DIAG and desc.R <= 32:
        return K.precond_build(L, d_t, constant_diag=const, root=desc.A0, perm=perm)
    return K.precond_build(L, d_t, constant_diag=const)


@pytest.mark.parametrize("N,R,B", [(2048, 32, 3), (8192, 32, 4), (1500, 8, 5), (4100, 16, 2)])
def test_preconditioner_build_rows_layout_matrix_core_path(N, R, B):
    """lo_precond_build_strided_f32 on the [B, m, N] rows the pivoted-Cholesky kernels write (fp64 MFMA Gram and
    Q kernels, no transposed copy) against the [B, N, k] streaming kernels and the golden reference values."""
    C, d, rhs = cases.lowrank_diag(301 if (N, R) == (2048, 32) else 5200 + R, B, N, R, 4)
    desc = K.lowrank_diag_descriptor(dev(C), None)
    Lc, _ = K.pivoted_cholesky(desc, 15)
    Lv, _ = K.pivoted_cholesky(desc, 15, contiguous=False)
    assert not Lv.is_contiguous() and torch.equal(Lc, Lv)
    sig = np.linspace(0.3, 1.1, B).astype(np.float32)
    for dd, const in ((dev(d), False), (dev(sig), True)):
        K._hip.prof_enable(True)
        pv = K.precond_build(Lv, dd, constant_diag=const)
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
        assert "pb_q_mfma" in prof and "pb_gram_mfma" in prof, "matrix-core path was not taken"
        pc = K.precond_build(Lc, dd, constant_diag=const)
        assert pv.k == pc.k and pv.Q.shape == pc.Q.shape
        assert np.allclose(host(pv.logdet), host(pc.logdet), rtol=1e-6)
        assert np.allclose(host(pv.dinv), host(pc.dinv), rtol=1e-7)
        # Q is fixed by the Cholesky factor of the SAME fp64 Gram matrix: equal up to fp64 summation order
        assert np.allclose(host(pv.Q), host(pc.Q), rtol=1e-5, atol=1e-6)
        zv, zc = host(K.precond_apply(pv, dev(rhs))), host(K.precond_apply(pc, dev(rhs)))
        assert max_rel_err_cols(zv, zc) < 2e-6
        if (N, R) == (2048, 32) and not const:
            g = load_golden("g3_precond")
            assert max_rel_err_cols(zv, g["z_nonconst"]) < 1e-5
            assert np.allclose(host(pv.logdet), g["logdet_nonconst"], rtol=1e-5)


@pytest.mark.parametrize("k", [3, 15, 16, 20, 32])
@pytest.mark.parametrize("const", [False, True])
def test_preconditioner_build_reference_layout_any_rank(k, const):
    """[B, N, k] factors (the Woodbury route hands its root over in this layout, k up to 32 on the fp64 matrix
    cores) against the oracle's fp64 QR construction."""
    B, N = 3, 3001
    rng = np.random.default_rng(7700 + k)
    L = (rng.standard_normal((B, N, k)) / np.sqrt(k)).astype(np.float32)
    d = (0.2 + rng.random((B, N))).astype(np.float32)
    sig = np.array([0.3, 0.7, 1.1], dtype=np.float32)
    rhs = rng.standard_normal((B, N, 4)).astype(np.float32)
    dd = np.broadcast_to(sig[:, None], (B, N)) if const else d
    K._hip.prof_enable(True)
    pre = K.precond_build(dev(L), dev(sig) if const else dev(d), constant_diag=const)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert "pb_q_mfma" in prof and "pb_gram_mfma" in prof
    po = orc.Preconditioner(L.astype(np.float64), dd.astype(np.float64))
    z = host(K.precond_apply(pre, dev(rhs)))
    assert max_rel_err_cols(z, po.apply(rhs.astype(np.float64))) < 1e-5
    assert np.allclose(host(pre.logdet), po.logdet, rtol=1e-5, atol=1e-3)
    # Q Q^T is unique (Q itself only up to an orthogonal factor)
    Q = host(pre.Q)[..., :k].astype(np.float64)
    if const:  # the device Q carries the 1/sqrt(sigma^2) of P^-1 = (I - Q Q^T) / sigma^2
        Q = Q * np.sqrt(sig.astype(np.float64))[:, None, None]
    assert np.allclose(Q @ np.swapaxes(Q, -1, -2) [:, :, :200], (po.Q @ np.swapaxes(po.Q, -1, -2))[:, :, :200], atol=2e-6)


def test_solve_lowrank_default_preconditioner():
    g = load_golden("g4_solve_lowrank")
    C, d, rhs = cases.lowrank_diag(401, 4, 2048, 32, 1)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
    assert res.iterations == int(g["matvecs"]) - 1 == 11 and res.tolerance_reached
    assert max_rel_err_cols(host(res.x), g["x"]) < 1e-4
    assert max_rel_err_cols(host(res.x), g["x_exact"]) < 1e-4


def test_inv_quad_logdet_lowrank_injected_probes():
    g = load_golden("g4_iql_lowrank")
    C, d, rhs = cases.lowrank_diag(411, 3, 2048, 16, 1)
    Z, _ = cases.probes(412, 3, 2048, 8)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    full = np.concatenate([Z, rhs], axis=-1)
    res = K.cg_solve(desc, dev(full), precond=pre, n_tridiag=8, tolerance=1e-4)
    assert res.iterations == int(g["matvecs"]) - 1 == 21
    assert max_rel_err_cols(host(res.x), g["solves"]) < 1e-4
    assert abs(res.t_mat.shape[-1] - g["t_mat"].shape[-1]) <= 1
    assert rel_err(host(res.t_mat)[..., :2, :2], g["t_mat"][..., :2, :2]) < 1e-4
    _, _, pinvk = K.tridiag_eigh_slq(res.t_mat, 2048)
    logdet = host(pinvk) + host(pre.logdet)
    inv_quad = (host(res.x)[..., 8:] * rhs).sum(-2)[..., 0]
    assert np.allclose(host(pre.logdet), g["logdet_p"], rtol=1e-5)
    assert np.allclose(inv_quad, g["inv_quad"], rtol=1e-4)
    floor = 2048 * 1.2e-7 * 137.0  # fp32 eigensolver noise floor of the REFERENCE
    assert np.allclose(logdet, g["logdet"], rtol=1e-4, atol=floor)
    # G7: eig + SLQ on the reference's own t_mat
    evals, evecs, pk = K.tridiag_eigh_slq(dev(g["t_mat"]), 2048, want_evecs=True)
    assert np.allclose(host(evals), g["evals"], rtol=1e-4, atol=1e-4)
    assert np.allclose(host(pk), g["pinvk_logdet"], rtol=1e-4, atol=floor)
    ev64, vec64 = np.linalg.eigh(g["t_mat"].astype(np.float64))
    assert np.allclose(host(evals), ev64, rtol=1e-5, atol=1e-5)
    slq64 = (2048 / 8.0) * (vec64[..., 0, :] ** 2 * np.log(ev64)).sum(-1).sum(0)
    assert np.allclose(host(pk), slq64, rtol=1e-4, atol=1e-3)
    rec = np.einsum("...ij,...j,...kj->...ik", host(evecs).astype(np.float64), host(evals).astype(np.float64),
                    host(evecs).astype(np.float64))
    assert np.allclose(rec, g["t_mat"], atol=1e-3)


def test_solve_kron_constant_diag():
    g = load_golden("g4_solve_kron")
    K1, K2, sig, rhs = cases.kron_factors(421, 2, 48, 48, 1)
    desc = K.kron_diag_descriptor(dev(K1), dev(K2), dev(sig[:, 0]), const_diag=True)
    pre = _default_precond(desc, dev(sig[:, 0]), True)
    res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-3)
    assert abs(res.iterations - (int(g["matvecs"]) - 1)) <= 3
    assert max_rel_err_cols(host(res.x), g["x"]) < 5e-3
    assert max_rel_err_cols(host(res.x), g["x_exact"]) < 2e-2


@pytest.mark.parametrize("tag,seed,n", [("n48", 421, 48), ("n128", 2201, 128)])
def test_solve_kron_iteration_pinned_1e4(tag, seed, n, monkeypatch):
    """cfg4 parity at the north_star bar: the HIP path runs EXACTLY the reference's iteration count (tolerance 0,
    max_iter = the count the reference needed at tolerance 1e-3; golden g22 holds the reference's iterate after that
    many iterations) and must agree per column to 1e-4 -- with the streaming engine's kernels under test: at
    128 (x) 128 the matrix-core Kronecker GEMMs (k_kron_nt_mfma) and the single-pass preconditioner apply
    (k_precond_fused), which the +-3-iteration stop-rule test above cannot pin to better than tol * cond."""
    g = load_golden("g22_kron_iteration_pinned")
    K1, K2, sig, rhs = cases.kron_factors(seed, 2, n, n, 1)
    its = int(g[f"iterations_{tag}"])
    desc = K.kron_diag_descriptor(dev(K1), dev(K2), dev(sig[:, 0]), const_diag=True)
    pre = _default_precond(desc, dev(sig[:, 0]), True)
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=0.0, max_iter=its)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert res.iterations == its and not res.tolerance_reached
    if n == 128:
        assert "kron_gemm_mfma" in prof and "precond_fused" in prof, f"kernels under test did not run: {sorted(prof)}"
    assert max_rel_err_cols(host(res.x), g[f"x_pinned_{tag}"]) < 1e-4
    # the same through the two-launch preconditioner apply (the fused apply's fallback): also within the bar
    monkeypatch.setenv("LO_NO_FUSED_PRECOND", "1")
    res2 = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=0.0, max_iter=its)
    assert res2.iterations == its and max_rel_err_cols(host(res2.x), g[f"x_pinned_{tag}"]) < 1e-4


def test_inv_quad_logdet_dense_injected_probes():
    g = load_golden("g4_iql_dense")
    Kd, d, rhs = cases.dense_diag(431, 2, 2048, 1)
    Z, _ = cases.probes(432, 2, 2048, 4)
    desc = K.dense_diag_descriptor(dev(Kd), dev(d))
    pre = _default_precond(desc, dev(d), False)
    res = K.cg_solve(desc, dev(np.concatenate([Z, rhs], -1)), precond=pre, n_tridiag=4, tolerance=1e-4)
    assert res.iterations == int(g["matvecs"]) - 1
    assert max_rel_err_cols(host(res.x), g["solves"]) < 1e-4
    _, _, pinvk = K.tridiag_eigh_slq(res.t_mat, 2048)
    logdet = host(pinvk) + host(pre.logdet)
    assert np.allclose((host(res.x)[..., 4:] * rhs).sum(-2)[..., 0], g["inv_quad"], rtol=1e-4)
    assert np.allclose(logdet, g["logdet"], rtol=1e-4, atol=2048 * 1.2e-7 * 10.0)


# ------------------------------------------------------------------------------------------- Lanczos
def test_lanczos_against_reference():
    g = load_golden("g5_lanczos")
    M = cases.spd_test_matrix(501, 100, dtype=np.float32, jitter=1e-6)
    v0 = cases.randn(502, 100, 1, dtype=np.float32)
    q, t = K.lanczos_tridiag(K.dense_diag_descriptor(dev(M[None]), None), dev(v0[None]), 100)
    q, t = host(q)[0], host(t)[0]
    assert q.shape[0] == 100 and t.shape[0] == t.shape[1] == q.shape[1]
    assert np.allclose(t[:10, :10], g["t_near"][:10, :10], rtol=1e-3, atol=1e-5)
    assert np.allclose(q @ t @ q.T, M, atol=1e-4)  # test_lanczos.py:35-36
    M2 = g["M_approx"]
    v2 = cases.randn(504, 30, 1, dtype=np.float32)
    Mt = dev(M2)
    q2, t2 = K.lanczos_tridiag(None, dev(v2), 30, matvec_closure=lambda v: Mt @ v)  # closure path
    q2, t2 = host(q2), host(t2)
    assert np.allclose(q2 @ t2 @ q2.T, M2, atol=1e-4)
    C, d, _ = cases.lowrank_diag(511, 2, 256, 8, 1)
    V = cases.randn(512, 2, 256, 3, dtype=np.float32)
    q3, t3 = K.lanczos_tridiag(K.lowrank_diag_descriptor(dev(C), dev(d)), dev(V), 10)
    assert tuple(q3.shape) == g["q_batch"].shape and tuple(t3.shape) == g["t_batch"].shape
    assert np.allclose(host(t3), g["t_batch"], rtol=1e-3, atol=1e-4)
    assert np.allclose(host(q3), g["q_batch"], atol=2e-3)


# ------------------------------------------------------------------------------------------- operator-resident CG
@pytest.mark.parametrize("N,R", [(8192, 32), (4096, 16), (2048, 8), (5000, 32), (4096, 20), (3000, 6), (20000, 32),
                                 (32768, 16)])  # (groups of 8 / 16 / 32 workgroups)
def test_onchip_cg_matches_streaming_engine_and_oracle(N, R):
    """The operator-resident fast path (8 workgroups per member, C in LDS, Q in VGPRs, granule all-reduces) runs the
    same arithmetic as the streaming engine: same iteration count, solutions equal to summation-order noise."""
    B = 70  # more members than the 32 concurrent groups, not a multiple of it
    C, d, rhs = cases.lowrank_diag(3100 + R, B, N, R, 1)
    rhs[3] = 0.0  # one all-zero right-hand side
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
        K.set_onchip_cg(True)
        _hip_prof = K._hip
        _hip_prof.prof_enable(True)
        res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
        torch.cuda.synchronize()
        prof = _hip_prof.prof_report()
        _hip_prof.prof_enable(False)
    finally:
        K.set_onchip_cg(True)
    assert "cg_onchip" in prof, "fast path was not taken"
    assert res.iterations == ref.iterations == 11 and res.tolerance_reached
    assert np.all(host(res.x)[3] == 0)
    keep = [i for i in range(B) if i != 3]
    assert max_rel_err_cols(host(res.x)[keep], host(ref.x)[keep]) < 2e-5
    sub = slice(0, 4)
    pre_o = orc.Preconditioner(host(K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C[sub]), None), 15)[0]), d[sub])
    xo, _, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C[sub], d[sub], v), rhs[sub], tolerance=1e-4,
                                preconditioner=pre_o.apply)
    assert info.iterations == res.iterations
    assert max_rel_err_cols(host(res.x)[:3], xo[:3]) < 1e-4
    # bitwise reproducible run to run (fixed summation order, no float atomics)
    res2 = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
    assert torch.equal(res.x, res2.x)


def _assert_tridiag_close(t_a, t_b, N, lead=2, same_size=True):
    """Two fp32 runs of the same recurrence: the leading block agrees entry by entry; once a column sits at its fp32
    noise floor alpha = r.z / p.Ap is a ratio of rounding noise, so the tail is compared through what it is used for --
    the SLQ log-determinant estimate (per-member, relative to N)."""
    a, b = host(t_a), host(t_b)
    # (a freeze one iteration apart -- an off-diagonal of 1e-6 +- rounding -- only appends noise-floor rows)
    assert a.shape[:-2] == b.shape[:-2] and abs(a.shape[-1] - b.shape[-1]) <= (0 if same_size else 1)
    m = min(lead, a.shape[-1], b.shape[-1])
    assert np.allclose(a[..., :m, :m], b[..., :m, :m], rtol=2e-3, atol=1e-4)
    _, _, ld_a = K.tridiag_eigh_slq(t_a.contiguous(), N)
    _, _, ld_b = K.tridiag_eigh_slq(t_b.contiguous(), N)
    assert np.abs(host(ld_a) - host(ld_b)).max() / N < 1e-4


@pytest.mark.usefixtures("legacy_resident_engines")
@pytest.mark.parametrize("N,R,c,nt", [(4096, 32, 5, 0), (8192, 32, 7, 6), (2048, 16, 3, 3), (5000, 8, 17, 16)])
def test_onchip_cg_many_columns_and_tridiagonals(N, R, c, nt):
    """Several right-hand-side columns (the inv_quad_logdet call: probes + rhs) run one after the other against the
    resident rows; the Lanczos tridiagonals are replayed from the recorded alpha / beta.  Same iteration count,
    solutions, tridiagonal blocks and last_tridiag_iter as the streaming engine, and the oracle on a sub-batch."""
    B = 41
    C, d, rhs = cases.lowrank_diag(4400 + c, B, N, R, c)
    rhs[2, :, 1] = 0.0  # an all-zero column
    if nt:
        rhs[..., :nt] /= np.maximum(np.linalg.norm(rhs[..., :nt], axis=-2, keepdims=True), 1e-30)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    kw = dict(precond=pre, tolerance=1e-4, n_tridiag=nt)
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, dev(rhs), **kw)
    finally:
        K.set_onchip_cg(True)
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), **kw)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert _resident_ran(prof) and not any(k.startswith("skinny_") for k in prof), "resident kernel alone expected"
    assert res.iterations == ref.iterations == (21 if nt else 11) and res.tolerance_reached
    assert np.all(host(res.x)[2, :, 1] == 0)
    x, xr = host(res.x), host(ref.x)
    mask = np.ones((B, c), bool)
    mask[2, 1] = False
    err = np.linalg.norm(x - xr, axis=-2) / np.maximum(np.linalg.norm(xr, axis=-2), 1e-30)
    assert err[mask].max() < 2e-5
    if nt:
        assert res.t_mat.shape == ref.t_mat.shape  # (same last_tridiag_iter)
        _assert_tridiag_close(res.t_mat, ref.t_mat, N)
    sub = slice(0, 3)
    pre_o = orc.Preconditioner(host(K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C[sub]), None), 15)[0]), d[sub])
    xo, to, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C[sub], d[sub], v), rhs[sub], tolerance=1e-4,
                                 preconditioner=pre_o.apply, n_tridiag=nt)
    erro = np.linalg.norm(x[sub] - xo, axis=-2) / np.maximum(np.linalg.norm(xo, axis=-2), 1e-30)
    assert erro[mask[sub]].max() < 1e-4
    if nt:  # (the freeze rule :326-327 is batch-global: the oracle's sub-batch needs its own device run)
        pre_s = _default_precond(K.lowrank_diag_descriptor(dev(C[sub]), dev(d[sub])), dev(d[sub]), False)
        rs = K.cg_solve(K.lowrank_diag_descriptor(dev(C[sub]), dev(d[sub])), dev(rhs[sub]), precond=pre_s,
                        tolerance=1e-4, n_tridiag=nt)
        _assert_tridiag_close(rs.t_mat, torch.from_numpy(to.astype(np.float32)).cuda(), N, same_size=False)
    res2 = K.cg_solve(desc, dev(rhs), **kw)
    assert torch.equal(res.x, res2.x) and (not nt or torch.equal(res.t_mat, res2.t_mat))


@pytest.mark.usefixtures("legacy_resident_engines")
@pytest.mark.parametrize("N,R,c,nt,mode", [
    (8192, 32, 16, 16, "full"),     # BASELINE cfg3 probes: one chunk of 16
    (8192, 32, 17, 16, "full"),     # cfg3 as written: 16 columns in lockstep + the 17th on the serial kernel
    (4096, 32, 33, 0, "full"),      # two chunks + one serial column
    (3000, 16, 5, 4, "full"),       # rank-16 root, partial chunk, ragged rows
    (2048, 8, 6, 0, "const"),       # rank-8 root (zero-padded to 16 on chip), constant diagonal
    (5000, 20, 20, 16, "full"),     # rank 20 (padded to 32), chunks of 16 + 4
    (4096, 32, 16, 0, "nopre"),     # no preconditioner: z = r
    (1500, 16, 9, 0, "nopre"),
])
def test_lockstep_cg_matches_serial_resident_streaming_and_oracle(N, R, c, nt, mode, monkeypatch):
    """The 16-column lockstep kernel (matrix cores, one all-reduce per iteration, lo_cg_lockstep.hip) against the
    serial-column resident kernel, the streaming engine and the oracle: same iteration count and last_tridiag_iter,
    solutions within summation-order noise of each other and within 1e-4 of the oracle, tridiagonals equivalent."""
    B = 37  # more work items than the 32 concurrent groups
    C, d, rhs = cases.lowrank_diag(5200 + c, B, N, R, c)
    rhs[2, :, 1] = 0.0  # an all-zero column
    if mode == "const":
        d = np.repeat(d[:, :1], N, axis=1)
    if nt:
        rhs[..., :nt] /= np.maximum(np.linalg.norm(rhs[..., :nt], axis=-2, keepdims=True), 1e-30)
    const = mode == "const"
    d_t = dev(d[:, 0]) if const else dev(d)  # constant diagonal: one value per member
    desc = K.lowrank_diag_descriptor(dev(C), d_t, const_diag=const)
    pre = None if mode == "nopre" else _default_precond(desc, d_t, const)
    kw = dict(precond=pre, tolerance=1e-4, n_tridiag=nt, max_iter=300)
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, dev(rhs), **kw)
    finally:
        K.set_onchip_cg(True)
    monkeypatch.setenv("LO_OC_NO_LOCKSTEP", "1")
    ser = K.cg_solve(desc, dev(rhs), **kw)
    monkeypatch.delenv("LO_OC_NO_LOCKSTEP")
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), **kw)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert "cg_lockstep" in prof, "lockstep kernel was not used"
    assert ("cg_onchip" in prof) == (c % 16 in (1, 2, 3)), "column split between the two resident kernels"
    if mode == "nopre":
        assert abs(res.iterations - ref.iterations) <= 1 and abs(ser.iterations - ref.iterations) <= 1
    else:
        assert res.iterations == ser.iterations == ref.iterations == (21 if nt else 11) and res.tolerance_reached
    x, xs, xr = host(res.x), host(ser.x), host(ref.x)
    assert np.all(x[2, :, 1] == 0)
    mask = np.ones((B, c), bool)
    mask[2, 1] = False

    def colerr(a, b):
        return (np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-30))[mask].max()

    # (without a preconditioner CG stops by tolerance, not at the floor: two fp32 summation orders may stop one
    # iteration apart, i.e. differ by a fraction of the 1e-4 tolerance)
    bar = 1e-4 if mode == "nopre" else 3e-5
    assert colerr(x, xs) < bar and colerr(x, xr) < bar
    if nt:
        assert res.t_mat.shape == ser.t_mat.shape == ref.t_mat.shape  # (same last_tridiag_iter)
        _assert_tridiag_close(res.t_mat, ref.t_mat, N)
        _assert_tridiag_close(res.t_mat, ser.t_mat, N)
    sub = slice(0, 3)
    if mode == "nopre":
        xo, _, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C[sub], d[sub], v), rhs[sub], tolerance=1e-4,
                                    max_iter=300)
    else:
        Lo = host(K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C[sub]), None), 15)[0])
        pre_o = orc.Preconditioner(Lo, d[sub])
        xo, _, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C[sub], d[sub], v), rhs[sub], tolerance=1e-4,
                                    preconditioner=pre_o.apply, n_tridiag=nt)
    erro = np.linalg.norm(x[sub] - xo, axis=-2) / np.maximum(np.linalg.norm(xo, axis=-2), 1e-30)
    assert erro[mask[sub]].max() < 1e-4
    res2 = K.cg_solve(desc, dev(rhs), **kw)  # bitwise reproducible run to run
    assert torch.equal(res.x, res2.x) and (not nt or torch.equal(res.t_mat, res2.t_mat))


@pytest.mark.usefixtures("legacy_resident_engines")
def test_lockstep_two_workgroups_per_cu_variant_matches_default(monkeypatch):
    """LO_LS_V2: 512-row workgroups, two per CU, groups of 16 with the reduce-scatter all-reduce -- same results as the
    default variant (different summation order across workgroups: compared to rounding noise) and reproducible."""
    C, d, rhs = cases.lowrank_diag(5301, 37, 8192, 32, 16)
    rhs /= np.linalg.norm(rhs, axis=-2, keepdims=True)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    kw = dict(precond=pre, tolerance=1e-4, n_tridiag=16)
    ref = K.cg_solve(desc, dev(rhs), **kw)
    monkeypatch.setenv("LO_LS_V2", "1")
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), **kw)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    res2 = K.cg_solve(desc, dev(rhs), **kw)
    assert "cg_lockstep" in prof and res.iterations == ref.iterations == 21
    assert max_rel_err_cols(host(res.x), host(ref.x)) < 2e-5 and res.t_mat.shape == ref.t_mat.shape
    _assert_tridiag_close(res.t_mat, ref.t_mat, 8192)
    assert torch.equal(res.x, res2.x) and torch.equal(res.t_mat, res2.t_mat)


@pytest.mark.usefixtures("legacy_resident_engines")
@pytest.mark.parametrize("N,R,c,nt,const", [(8192, 32, 1, 0, False), (4096, 16, 3, 2, False), (5000, 20, 2, 0, True),
                                            (20000, 32, 1, 0, False), (2048, 8, 1, 1, True)])
def test_root_form_preconditioner_and_serial_kernel(N, R, c, nt, const, monkeypatch):
    """The root form of the pivoted-Cholesky preconditioner (P^-1 r = (r - C F C^T (r/d)) / d, lo_precond_root_form_f32)
    is the same operator as the Q form (same logdet, same apply), and the serial-column resident kernel built on it (one
    all-reduce per iteration) gives the iterations / solutions / tridiagonals of the Q-form kernel and of the streaming
    engine.  A root-form-ONLY preconditioner (no Q) works whenever the resident kernel takes the solve and rebuilds Q
    on demand otherwise."""
    B = 37
    C, d, rhs = cases.lowrank_diag(5400 + R, B, N, R, c)
    if const:
        d = np.repeat(d[:, :1], N, axis=1)
    if nt:
        rhs[..., :nt] /= np.linalg.norm(rhs[..., :nt], axis=-2, keepdims=True)
    d_t = dev(d[:, 0]) if const else dev(d)
    desc = K.lowrank_diag_descriptor(dev(C), d_t, const_diag=const)
    L, perm = K.pivoted_cholesky(desc, 15)
    pre_q = K.precond_build(L, d_t, const)
    pre_r = K.precond_build(L, d_t, const, root=desc.A0, perm=perm)
    assert pre_r.F is not None and pre_r.Q is not None and pre_r.rf_ld == K.padded_rank(R)
    assert np.allclose(host(pre_r.logdet), host(pre_q.logdet), rtol=2e-6)
    # the two forms are the same operator: apply the root form by hand
    v = dev(rhs)
    dinv = pre_r.dinv.unsqueeze(-1) if not const else pre_r.dinv.reshape(B, 1, 1)
    Cp = torch.nn.functional.pad(dev(C), (0, pre_r.rf_ld - R))
    z_root = (v - Cp @ (pre_r.F @ (Cp.mT @ (v * dinv)))) * dinv
    assert max_rel_err_cols(host(z_root), host(K.precond_apply(pre_q, v))) < 5e-6
    assert torch.allclose(pre_r.EF, pre_r.E @ pre_r.F, rtol=1e-4, atol=1e-6)
    kw = dict(tolerance=1e-4, n_tridiag=nt)
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, v, precond=pre_q, **kw)
    finally:
        K.set_onchip_cg(True)
    res_q = K.cg_solve(desc, v, precond=pre_q, **kw)        # Q-form resident kernel (no root form to take)
    assert K.cg_last_executed()["serial_engine"] == "gen2"
    K._hip.prof_enable(True)
    res_r = K.cg_solve(desc, v, precond=pre_r, **kw)        # root-form resident kernel
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert "cg_onchip" in prof and not any(k.startswith("skinny_") for k in prof)
    assert res_r.iterations == res_q.iterations == ref.iterations == (21 if nt else 11) and res_r.tolerance_reached
    assert max_rel_err_cols(host(res_r.x), host(ref.x)) < 3e-5 and max_rel_err_cols(host(res_r.x), host(res_q.x)) < 3e-5
    if nt:
        assert res_r.t_mat.shape == ref.t_mat.shape
        _assert_tridiag_close(res_r.t_mat, ref.t_mat, N)
    assert torch.equal(res_r.x, K.cg_solve(desc, v, precond=pre_r, **kw).x)  # reproducible
    # root form only
    pre_o = K.precond_build(L, d_t, const, root=desc.A0, perm=perm, need_q=False)
    assert pre_o.Q is None
    res_o = K.cg_solve(desc, v, precond=pre_o, **kw)
    assert torch.equal(res_o.x, res_r.x) and pre_o.Q is None
    try:  # ... and when the resident kernels are off the Q form is built on demand
        K.set_onchip_cg(False)
        res_f = K.cg_solve(desc, v, precond=pre_o, **kw)
    finally:
        K.set_onchip_cg(True)
    assert pre_o.Q is not None and max_rel_err_cols(host(res_f.x), host(ref.x)) < 1e-6


@pytest.mark.parametrize("kind,N", [("dense", 8192), ("kron", 16384), ("dense", 10000), ("kron", 65536)])
def test_fused_preconditioner_apply_matches_two_pass_path(kind, N, monkeypatch):
    """Single-column CG on large operators that are not resident (dense, Kronecker): the preconditioner apply fused with
    the r / x update reads Q once per iteration (lo_precond_fused.hip, groups of 16-64 workgroups, one all-reduce); same
    iteration count and solution as the two-launch path, bitwise reproducible."""
    B = 5 if N < 65536 else 19
    if kind == "dense":
        K0, d, rhs = cases.dense_diag(5600 + N % 97, B, N, 1)
        d_t = dev(d)
        desc = K.dense_diag_descriptor(dev(K0), d_t)
        const = False
    else:
        n = int(round(N ** 0.5))
        K1, K2, sig, rhs = cases.kron_factors(5700, B, n, n, 1)
        d_t = dev(sig[:, 0])
        desc = K.kron_diag_descriptor(dev(K1), dev(K2), d_t, const_diag=True)
        const = True
    L, _ = K.pivoted_cholesky(desc, 15)
    pre = K.precond_build(L, d_t, const)
    kw = dict(precond=pre, tolerance=1e-3, max_iter=400)
    monkeypatch.setenv("LO_NO_FUSED_PRECOND", "1")
    ref = K.cg_solve(desc, dev(rhs), **kw)
    monkeypatch.delenv("LO_NO_FUSED_PRECOND")
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), **kw)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    # (the initial z = P^-1 r of linear_cg.py:213 still takes the two-launch path: one skinny pair in the profile)
    assert prof.get("precond_fused", (0, 0))[0] >= res.iterations - 1 and prof.get("skinny_tn_R16", (0, 0))[0] <= 1
    assert abs(res.iterations - ref.iterations) <= 1 and res.tolerance_reached == ref.tolerance_reached
    assert max_rel_err_cols(host(res.x), host(ref.x)) < 1e-4
    res2 = K.cg_solve(desc, dev(rhs), **kw)
    assert torch.equal(res.x, res2.x) and res2.iterations == res.iterations
    # the iteration's control step (beta, residual norms, has_converged, the batch-global stop rule) rides in the same
    # launch from the second iteration on: no control kernel in the profile but the first one, and exactly the
    # iterations, flags and solution of the separate control kernels
    assert prof.get("cg_ctrl", (0, 0))[0] <= 1, prof.get("cg_ctrl")
    monkeypatch.setenv("LO_NO_FUSED_CTRL", "1")
    sep = K.cg_solve(desc, dev(rhs), **kw)
    monkeypatch.delenv("LO_NO_FUSED_CTRL")
    assert sep.iterations == res.iterations and sep.tolerance_reached == res.tolerance_reached
    assert torch.equal(sep.x, res.x) and abs(sep.mean_residual - res.mean_residual) <= 1e-6 * abs(sep.mean_residual)


def test_onchip_cg_many_columns_hand_over():
    """Columns + tridiagonals + a tolerance the guaranteed iterations do not reach: the streaming loop continues from
    the resident kernel's per-column state."""
    C, d, rhs = cases.lowrank_diag(4490, 12, 4096, 32, 4)
    d = (10.0 ** (3.0 * (d - 0.5) - 2.0)).astype(np.float32)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    L, _ = K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C), None), 2)
    pre = K.precond_build(L, dev(d), False)
    kw = dict(precond=pre, tolerance=1e-5, max_iter=400, n_tridiag=3, max_tridiag_iter=8)  # 11 guaranteed iterations
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, dev(rhs), **kw)
    finally:
        K.set_onchip_cg(True)
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), **kw)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert _resident_ran(prof) and any(k.startswith("skinny_") for k in prof), "both engines must have run"
    assert ref.iterations > 11 and res.iterations > 11 and abs(res.iterations - ref.iterations) <= 4
    assert res.tolerance_reached == ref.tolerance_reached and res.t_mat.shape == ref.t_mat.shape
    assert max_rel_err_cols(host(res.x), host(ref.x)) < 1e-3
    _assert_tridiag_close(res.t_mat, ref.t_mat, 4096, lead=4)


# ------------------------------------------------------------------------------------------- many columns (MFMA paths)
@pytest.mark.parametrize("N,R", [(1500, 16), (4096, 32)])
def test_onchip_cg_without_preconditioner(N, R):
    """N < min_preconditioning_size in the host API means linear_cg gets no preconditioner: the resident kernel then
    runs with Q = 0, 1/d = 1 (z = r), the reference's unpreconditioned update (linear_cg.py:49-95): same iterations and
    solutions as the streaming engine and the oracle, including the hand-over when 11 iterations are not enough."""
    B = 37
    C, d, rhs = cases.lowrank_diag(3980 + R, B, N, R, 1)
    rhs[5] = 0.0
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    for tol in (1e-1, 1e-4):
        try:
            K.set_onchip_cg(False)
            ref = K.cg_solve(desc, dev(rhs), tolerance=tol, max_iter=300)
        finally:
            K.set_onchip_cg(True)
        K._hip.prof_enable(True)
        res = K.cg_solve(desc, dev(rhs), tolerance=tol, max_iter=300)
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
        assert "cg_onchip" in prof, "resident kernel was not used"
        assert abs(res.iterations - ref.iterations) <= 1 and res.tolerance_reached == ref.tolerance_reached
        keep = [i for i in range(B) if i != 5]
        assert np.all(host(res.x)[5] == 0)
        assert max_rel_err_cols(host(res.x)[keep], host(ref.x)[keep]) < 5e-5
    sub = slice(0, 3)
    xo, _, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C[sub], d[sub], v), rhs[sub], tolerance=1e-4,
                                max_iter=300)
    assert abs(info.iterations - res.iterations) <= 1
    assert max_rel_err_cols(host(res.x)[sub], xo) < 1e-4


def test_onchip_cg_hands_over_to_streaming_loop_beyond_the_floor():
    """When the tolerance is not met after the 11 guaranteed iterations the resident kernel's state (x, r, p, z and the
    per-member scalars) continues in the streaming loop: same iteration count and solution as the streaming engine
    alone, for a weak preconditioner (rank 2) and a tight tolerance."""
    C, d, rhs = cases.lowrank_diag(3950, 20, 4096, 32, 1)
    d = (10.0 ** (3.0 * (d - 0.5) - 2.0)).astype(np.float32)  # diagonal spread over 1e-2 .. 1e1: slow convergence
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    L, _ = K.pivoted_cholesky(K.lowrank_diag_descriptor(dev(C), None), 2)
    pre = K.precond_build(L, dev(d), False)
    try:
        K.set_onchip_cg(False)
        ref = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-5, max_iter=400)
    finally:
        K.set_onchip_cg(True)
    K._hip.prof_enable(True)
    res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-5, max_iter=400)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert "cg_onchip" in prof and any(k.startswith("skinny_") for k in prof), "both engines must have run"
    # (ill-conditioned on purpose, cond ~ 1e5: the fp32 convergence histories of the two summation orders differ by a
    # couple of iterations; both meet the tolerance)
    assert ref.iterations > 11 and res.iterations > 11 and abs(res.iterations - ref.iterations) <= 4
    assert res.tolerance_reached == ref.tolerance_reached
    assert max_rel_err_cols(host(res.x), host(ref.x)) < 1e-3  # ill-conditioned on purpose: cond ~ 1e5
    xo = orc.woodbury_solve(C.astype(np.float64), d.astype(np.float64), rhs.astype(np.float64))  # exact, fp64
    assert max_rel_err_cols(host(res.x), xo) < 5e-2


@pytest.mark.usefixtures("legacy_resident_engines")
def test_onchip_timeout_falls_back_to_streaming_engines(monkeypatch):
    """A timed-out group hand-off (error word set) makes the host redo the work with the streaming engines: same
    pivots / L bit for bit, same iteration count, solutions equal to summation-order noise."""
    C, d, rhs = cases.lowrank_diag(3900, 9, 4096, 32, 1)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    L0, p0 = K.pivoted_cholesky(desc, 15)
    pre = K.precond_build(L0, dev(d), False)
    ref = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
    monkeypatch.setenv("LO_OC_TEST_FALLBACK", "1")
    K._hip.prof_enable(True)
    L1, p1 = K.pivoted_cholesky(desc, 15)
    res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
    torch.cuda.synchronize()
    prof = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert "pc_update" in prof and any(k.startswith("skinny_tn") for k in prof), "streaming engines did not run"
    assert torch.equal(L0, L1) and torch.equal(p0, p1)
    assert res.iterations == ref.iterations and res.tolerance_reached
    assert max_rel_err_cols(host(res.x), host(ref.x)) < 2e-5
    # several columns with tridiagonals: the aborted resident attempt (its replay kernels ran on unusable records) must
    # leave nothing behind in the returned tridiagonals
    monkeypatch.delenv("LO_OC_TEST_FALLBACK")
    C5, d5, rhs5 = cases.lowrank_diag(3901, 6, 4096, 32, 5)
    rhs5[..., :4] /= np.linalg.norm(rhs5[..., :4], axis=-2, keepdims=True)
    desc5 = K.lowrank_diag_descriptor(dev(C5), dev(d5))
    pre5 = _default_precond(desc5, dev(d5), False)
    ref5 = K.cg_solve(desc5, dev(rhs5), precond=pre5, tolerance=1e-4, n_tridiag=4)
    monkeypatch.setenv("LO_OC_TEST_FALLBACK", "1")
    K._hip.prof_enable(True)
    res5 = K.cg_solve(desc5, dev(rhs5), precond=pre5, tolerance=1e-4, n_tridiag=4)
    torch.cuda.synchronize()
    prof5 = K._hip.prof_report()
    K._hip.prof_enable(False)
    assert _resident_ran(prof5) and any(k.startswith("skinny_") for k in prof5)
    assert res5.iterations == ref5.iterations == 21 and res5.t_mat.shape == ref5.t_mat.shape
    assert max_rel_err_cols(host(res5.x), host(ref5.x)) < 2e-5
    _assert_tridiag_close(res5.t_mat, ref5.t_mat, 4096)


def test_cg_many_columns_mfma_paths_vs_oracle():
    """cfg3 / cfg5-shaped right-hand sides (16 probes + 1 rhs) go through the v_mfma_f32_32x32x2_f32 kernels
    (lo_skinny_mfma.hip, lo_dense_mfma.hip): same iteration counts and solutions as the oracle."""
    # low-rank + diag, preconditioned, tridiagonals of the 16 probe columns
    C, d, rhs = cases.lowrank_diag(5101, 3, 2304, 32, 17)
    rhs[..., :16] /= np.sqrt((rhs[..., :16] ** 2).sum(-2, keepdims=True))
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    try:  # (the resident kernel would take this shape: the streaming matrix-core engine is what is under test here)
        K.set_onchip_cg(False)
        K._hip.prof_enable(True)
        res = K.cg_solve(desc, dev(rhs), precond=pre, n_tridiag=16, tolerance=1e-4)
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
    finally:
        K.set_onchip_cg(True)
    assert any(k.startswith("skinny_tn_mfma") for k in prof) and "cg_onchip" not in prof
    Lo, _ = orc.pivoted_cholesky(orc.LowRankRowSource(C), 15)
    po = orc.Preconditioner(Lo, d)
    xo, to, info = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C, d, v), rhs, n_tridiag=16, tolerance=1e-4,
                                 preconditioner=po.apply)
    assert res.iterations == info.iterations == 21
    assert max_rel_err_cols(host(res.x), xo) < 1e-4
    assert rel_err(host(res.t_mat)[..., :2, :2], to[..., :2, :2]) < 1e-4
    _, _, ld = K.tridiag_eigh_slq(res.t_mat, 2304)
    ev, evec = orc.lanczos_tridiag_to_diag(to.astype(np.float64))
    assert np.allclose(host(ld), orc.slq_logdet(2304, ev, evec), rtol=1e-4, atol=2304 * 1.2e-7 * 150)
    # unpreconditioned, 12 columns, R = 16 (padded operand tile half empty)
    C2, d2, rhs2 = cases.lowrank_diag(5102, 2, 1500, 16, 12)
    r2 = K.cg_solve(K.lowrank_diag_descriptor(dev(C2), dev(d2)), dev(rhs2), tolerance=1.0)
    x2, _, i2 = orc.linear_cg(lambda v: orc.matvec_lowrank_diag(C2, d2, v), rhs2, tolerance=1.0)
    assert r2.iterations == i2.iterations == 11 and max_rel_err_cols(host(r2.x), x2) < 1e-4
    # dense + diag, 17 columns, N not a multiple of the 128-row / 64-column tiles
    Kd, dd, rhs3 = cases.dense_diag(5103, 2, 1100, 17)
    desc3 = K.dense_diag_descriptor(dev(Kd), dev(dd))
    y = host(K.matvec(desc3, dev(rhs3)))
    assert max_rel_err_cols(y, orc.matvec_dense_diag(Kd.astype(np.float64), dd.astype(np.float64),
                                                     rhs3.astype(np.float64))) < 5e-6
    r3 = K.cg_solve(desc3, dev(rhs3), tolerance=1e-2, n_tridiag=4)
    x3, t3, i3 = orc.linear_cg(lambda v: orc.matvec_dense_diag(Kd, dd, v), rhs3, tolerance=1e-2, n_tridiag=4)
    assert abs(r3.iterations - i3.iterations) <= 1 and max_rel_err_cols(host(r3.x), x3) < 2e-3
    # 40 columns: two MFMA column tiles for the dense kernel, VALU chunks for the skinny kernels
    rhs4 = cases.randn(5104, 2, 1100, 40, dtype=np.float32)
    y4 = host(K.matvec(desc3, dev(rhs4)))
    assert max_rel_err_cols(y4, orc.matvec_dense_diag(Kd.astype(np.float64), dd.astype(np.float64),
                                                      rhs4.astype(np.float64))) < 5e-6
    C5, d5, rhs5 = cases.lowrank_diag(5105, 2, 900, 32, 40)
    y5 = host(K.matvec(K.lowrank_diag_descriptor(dev(C5), dev(d5)), dev(rhs5)))
    assert max_rel_err_cols(y5, orc.matvec_lowrank_diag(C5.astype(np.float64), d5.astype(np.float64),
                                                        rhs5.astype(np.float64))) < 5e-6


# ------------------------------------------------------------------------------------------- bilinear derivative (root)
@pytest.mark.parametrize("N,R,D", [(1001, 32, 2), (2048, 32, 34), (777, 5, 17), (1500, 20, 64), (900, 8, 70),
                                    (600, 40, 6)])
def test_bilinear_derivative_root_all_engines(N, R, D):
    """lo_bilinear_root_f32 = U (V^T C) + V (U^T C): matrix-core first phase for R <= 32, D <= 64 (one or two column
    tiles), VALU kernel beyond, against the oracle in fp64."""
    B = 3
    rng = np.random.default_rng(8800 + D)
    C = rng.standard_normal((B, N, R)).astype(np.float32)
    U = rng.standard_normal((B, N, D)).astype(np.float32)
    V = rng.standard_normal((B, N, D)).astype(np.float32)
    out = host(K.bilinear_root(dev(C), dev(U), dev(V)))
    ref = orc.bilinear_derivative_root(C.astype(np.float64), U.astype(np.float64), V.astype(np.float64))
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() <= 2e-5 * np.abs(ref).max()
    # the Diag derivative of the same factors from the same pass
    out2, rowdot = K.bilinear_root(dev(C), dev(U), dev(V), with_rowdot=True)
    assert torch.equal(out2, dev(out))
    rd = orc.bilinear_derivative_diag(U.astype(np.float64), V.astype(np.float64))
    assert np.abs(host(rowdot) - rd).max() <= 2e-5 * np.abs(rd).max()


@pytest.mark.parametrize("k", [33, 40, 64, 100, 128])
def test_wide_preconditioner_rank_above_32(k):
    """`max_preconditioner_size` beyond the register-resident k <= 32 algebra: tiled fp64 Gram, packed Cholesky and
    triangular inverse in LDS, Q = W T^-T (lo_precond.hip, k_pbw_*).  Pivots bit-exact, apply and logdet against the
    oracle's fp64 QR form, and CG with it reaches the exact solution in fewer iterations than without."""
    for const in (False, True):
        Kd, d, rhs = cases.dense_diag(9100 + k, 2, 1100, 3)
        if const:
            d = np.broadcast_to(d[:, :1], d.shape).copy()
        L, piv = K.pivoted_cholesky(K.dense_diag_descriptor(dev(Kd), None), k)
        Lo, pivo = orc.pivoted_cholesky(orc.DenseRowSource(Kd), k)
        assert np.array_equal(host(piv), pivo) and np.array_equal(host(L), Lo)
        darg = dev(d[:, 0].copy()) if const else dev(d)
        pre_o = orc.Preconditioner(Lo.astype(np.float64), d.astype(np.float64))
        for layout in ("nk", "rows"):
            if layout == "rows":
                L, _ = K.pivoted_cholesky(K.dense_diag_descriptor(dev(Kd), None), k, contiguous=False)
            pre = K.precond_build(L, darg, const)
            z = host(K.precond_apply(pre, dev(rhs)))
            assert max_rel_err_cols(z, pre_o.apply(rhs.astype(np.float64))) < 5e-5, (k, const, layout)
            assert np.allclose(host(pre.logdet), pre_o.logdet, rtol=1e-5), (k, const, layout)
        desc = K.dense_diag_descriptor(dev(Kd), darg, const_diag=const)
        res = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-5, max_iter=300)
        res0 = K.cg_solve(desc, dev(rhs), tolerance=1e-5, max_iter=300)
        A = Kd.astype(np.float64) + np.stack([np.diag(v) for v in d.astype(np.float64)])
        assert max_rel_err_cols(host(res.x), np.linalg.solve(A, rhs.astype(np.float64))) < 1e-4
        assert res.iterations <= res0.iterations


@pytest.mark.usefixtures("legacy_resident_engines")
@pytest.mark.parametrize("c,nt", [(1, 0), (17, 16), (3, 0)])
def test_result_only_first_pass_and_its_repeat_with_state(c, nt, monkeypatch):
    """The resident CG kernels first run result-only (no x / r / p / z of a possible continuation).  (i) At the floor
    the result is bit-identical to a run that writes the state (LO_OC_KEEP_STATE=1).  (ii) With a tolerance the floor
    cannot meet the launches are repeated with the state and the streaming engine continues from it: again
    bit-identical to the run that wrote the state in its first pass, same iteration count."""
    C, d, rhs = cases.lowrank_diag(9100 + c, 12, 8192, 32, c)
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    pre = _default_precond(desc, dev(d), False)
    if c == 1:  # (round 4: the result-only pass of ONE column carries w by recurrence -- another rounding sequence; it
        # agrees with the three-pass iteration to a few ulps of the solution: tests/test_gpu_parity_r4.py.  The bit
        # identities below are the lean / state mechanism's, checked on the three-pass kernel)
        wr = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
        monkeypatch.setenv("LO_OC_NO_WREC", "1")
        tp = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=1e-4)
        assert wr.iterations == tp.iterations == 11 and max_rel_err_cols(host(wr.x), host(tp.x)) < 5e-6
    for tol, max_iter in ((1e-4, 1000), (1e-9, 40)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            monkeypatch.delenv("LO_OC_KEEP_STATE", raising=False)
            K._hip.prof_enable(True)
            a = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=tol, n_tridiag=nt, max_iter=max_iter)
            torch.cuda.synchronize()
            prof = K._hip.prof_report()
            K._hip.prof_enable(False)
            monkeypatch.setenv("LO_OC_KEEP_STATE", "1")
            b = K.cg_solve(desc, dev(rhs), precond=pre, tolerance=tol, n_tridiag=nt, max_iter=max_iter)
        resident = prof.get("cg_onchip", (0, 0))[0] + prof.get("cg_lockstep", (0, 0))[0]
        assert resident >= 1, sorted(prof)
        assert a.iterations == b.iterations and a.tolerance_reached == b.tolerance_reached
        if tol == 1e-9:
            assert a.iterations > (21 if nt else 11)  # the streaming engine continued
            launches = (1 if c != 17 else 2)
            assert resident == 2 * launches, (resident, sorted(prof))  # result-only pass + the repeat with the state
        assert torch.equal(a.x, b.x)
        if nt:
            assert torch.equal(a.t_mat, b.t_mat)
