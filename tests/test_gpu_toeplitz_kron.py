"""Kronecker product of 2 or 3 Toeplitz factors on the MI355X: the column gradients of csrc/lo_ski_grid.hip against an
fp64 closed form, the LO_OP_TOEPLITZ_KRON_DIAG kind through lo_matvec_f32, `_matmul`, CG, Lanczos, MINRES, the pivoted
Cholesky and inv_quad_logdet with its backward against the reference's goldens (tests/golden/g36_toeplitz_kron.npz)."""
import ctypes as C
import math
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import column, rng  # noqa: E402
from make_golden_ski_grid import PC_RANK  # noqa: E402
from make_golden_toeplitz_kron import CASES, inputs  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.functions import pivoted_cholesky  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator,
    ToeplitzLinearOperator)
from linear_operator_amd.operators import kronecker_product_linear_operator as kpm  # noqa: E402

pytestmark = pytest.mark.gpu
X = inputs()
G = np.load(os.path.join(HERE, "golden", "g36_toeplitz_kron.npz"))
GUARD = 1024  # sentinel floats before and after g and the workspace
KIND = K._hip.LO_OP_TOEPLITZ_KRON_DIAG


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def close(a, b, rel=3e-3):
    a, b = host(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * np.abs(b).max()


def kron(p, cols=None):
    D = len(CASES[p][0]) if p in CASES else 2
    cols = [dev(X[f"{p}_c{k + 1}"]) for k in range(D)] if cols is None else cols
    return KroneckerProductLinearOperator(*[ToeplitzLinearOperator(c) for c in cols])


def grads64(cols, u, v):
    """The column gradients of one member in fp64, by the closed form on dense per-axis matrices: W_k = v with every
    factor but T_k applied, g_k[l] = sum over the other axes and s of the lag-l correlation of u and W_k along axis k."""
    grid = [t.shape[-1] for t in cols]
    S = u.shape[-1]
    mats = [t.astype(np.float64)[np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])] for t, m in zip(cols, grid)]
    u = u.astype(np.float64).reshape(*grid, S)
    out = []
    for k, m in enumerate(grid):
        w = v.astype(np.float64).reshape(*grid, S)
        for j, Tj in enumerate(mats):
            if j != k:
                w = np.moveaxis(np.tensordot(Tj, w, axes=(1, j)), 0, j)
        uk = np.moveaxis(u, k, 0).reshape(m, -1)
        wk = np.moveaxis(w, k, 0).reshape(m, -1)
        g = np.zeros(m)
        for l in range(m):
            g[l] = (uk[:m - l] * wk[l:]).sum() + ((uk[l:] * wk[:m - l]).sum() if l else 0.0)
        out.append(g)
    return out


def bilinear_inputs(grid, S, B):
    cols = [column(3900 + k, B, m, ls=0.2) * (1.0 + 0.1 * rng(3910 + k).standard_normal((B, m))).astype(np.float32)
            for k, m in enumerate(grid)]
    M = int(np.prod(grid))
    u = rng(3920 + M).standard_normal((B, M, S)).astype(np.float32)
    v = rng(3930 + M).standard_normal((B, M, S)).astype(np.float32)
    return cols, u, v


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def bits(t):
    return t.view(torch.int32)


def guarded_bilinear(cols, u, v):
    """lo_toeplitz_kron_bilinear_f32 the way K.toeplitz_kron_bilinear launches it, with g and the workspace between
    NaN guard bands.  Returns (g on the host, whether the four guard bands kept their bits)."""
    lib = K._hip.load()
    grid = [t.shape[-1] for t in cols]
    B, M, S = u.shape
    m = (C.c_int64 * len(grid))(*grid)
    ws_bytes = lib.lo_toeplitz_kron_bilinear_workspace_bytes(m, len(grid), B, S)
    assert ws_bytes > 0
    nws = (ws_bytes + 3) // 4
    gbuf, gv = guarded(B * sum(grid))
    wbuf, wv = guarded(nws)
    K._launch("lo_toeplitz_kron_bilinear_f32", gbuf.device, dev(np.concatenate(cols, -1)), m, len(grid), B, dev(u),
              dev(v), S, gv, wv, ws_bytes)
    torch.cuda.synchronize()
    sentinel = bits(torch.full((GUARD,), float("nan"), dtype=torch.float32, device="cuda"))
    intact = all(torch.equal(bits(b[:GUARD]), sentinel) and torch.equal(bits(b[-GUARD:]), sentinel)
                 for b in (gbuf, wbuf))
    return host(gv).reshape(B, sum(grid)), intact


@pytest.mark.parametrize("grid,S,B", [((5, 7), 1, 1), ((1, 8), 2, 1), ((33, 20), 3, 1), ((130, 65), 17, 2),
                                      ((6, 5, 4), 2, 1), ((17, 9, 33), 5, 1), ((1024, 3), 1, 1), ((3, 1024), 2, 1)])
def test_column_gradients_against_the_fp64_closed_form(grid, S, B):
    cols, u, v = bilinear_inputs(grid, S, B)
    g1, intact1 = guarded_bilinear(cols, u, v)
    g2, intact2 = guarded_bilinear(cols, u, v)
    api = K.toeplitz_kron_bilinear([dev(t) for t in cols], dev(u), dev(v))
    assert intact1 and intact2, "the kernels wrote outside g or the workspace"
    assert np.array_equal(g1.view(np.int32), g2.view(np.int32))
    assert np.array_equal(np.concatenate([host(a) for a in api], -1).view(np.int32), g1.view(np.int32))
    off = 0
    for k, m in enumerate(grid):
        for b in range(B):
            ref = grads64([t[b] for t in cols], u[b], v[b])[k]
            err = np.linalg.norm(g1[b, off:off + m] - ref) / np.linalg.norm(ref)
            print(f"bilinear {grid} S={S} B={B} axis {k} member {b}: rel err {err:.3e}")
            assert err <= 1e-4
        off += m


def test_entry_points_refuse_what_they_do_not_take():
    lib = K._hip.load()
    t = torch.ones(16, device="cuda")
    u = torch.zeros(256, device="cuda")
    ws = torch.zeros(1 << 16, device="cuda")
    st = K._hip.stream_ptr(u.device)
    m4 = (C.c_int64 * 4)(4, 4, 4, 4)
    assert lib.lo_toeplitz_kron_bilinear_workspace_bytes(m4, 4, 1, 1) == 0
    assert lib.lo_toeplitz_kron_bilinear_f32(K._hip.ptr(t), m4, 4, 1, K._hip.ptr(u), K._hip.ptr(u), 1, K._hip.ptr(t),
                                             K._hip.ptr(ws), ws.numel() * 4, st) == K._hip.LO_ERR_UNSUPPORTED
    m2 = (C.c_int64 * 2)(4, 4)
    assert lib.lo_toeplitz_kron_bilinear_f32(None, m2, 2, 1, K._hip.ptr(u), K._hip.ptr(u), 1, K._hip.ptr(t),
                                             K._hip.ptr(ws), ws.numel() * 4, st) == -1  # LO_ERR_BADARG
    wide = (C.c_int64 * 2)(1025, 2)
    assert lib.lo_toeplitz_kron_bilinear_workspace_bytes(wide, 2, 1, 1) == 0


@pytest.mark.parametrize("p", list(CASES))
def test_kind_through_matvec_and_matmul_against_goldens(p):
    grid, B = CASES[p]
    A = kron(p)
    desc = A._kernel_descriptor()
    assert desc.kind == KIND and desc.grid == grid and desc.B == B and desc.N == math.prod(grid)
    d = dev(X[p + "_d"])
    sigma = dev(np.linspace(0.5, 1.5, B).astype(np.float32).reshape(B, 1))
    full = AddedDiagLinearOperator(A, DiagLinearOperator(d))
    const = AddedDiagLinearOperator(A, ConstantDiagLinearOperator(sigma, diag_shape=desc.N))
    assert full._kernel_descriptor().diag_mode == K._hip.LO_DIAG_FULL
    assert const._kernel_descriptor().diag_mode == K._hip.LO_DIAG_CONST
    for c in (1, 5):
        rhs, ref = dev(X[f"{p}_rhs{c}"]), G[f"{p}_mm{c}"]
        assert np.allclose(host(K.matvec(desc, rhs)), ref, rtol=1e-4, atol=1e-5)
        assert np.allclose(host(A._matmul(rhs)), ref, rtol=1e-4, atol=1e-5)
        for table in ({}, {(len(grid), 1): True, (len(grid), 2): True}):  # both routes of `_matmul`
            with mock.patch.object(kpm, "_NATIVE_MATMUL_TOEPLITZ", table):
                assert np.allclose(host(A._matmul(rhs)), ref, rtol=1e-4, atol=1e-5)
        r = X[f"{p}_rhs{c}"]
        assert np.allclose(host(K.matvec(full._kernel_descriptor(), rhs)), ref + X[p + "_d"][..., None] * r, rtol=1e-4,
                           atol=1e-5)
        assert np.allclose(host(K.matvec(const._kernel_descriptor(), rhs)), ref + host(sigma)[..., None] * r,
                           rtol=1e-4, atol=1e-5)


def test_diagonal_in_the_last_pass_and_as_an_epilogue_agree():
    desc = AddedDiagLinearOperator(kron("g3"), DiagLinearOperator(dev(X["g3_d"])))._kernel_descriptor()
    rhs = dev(X["g3_rhs5"])
    y = host(K.matvec(desc, rhs))
    with mock.patch.dict(os.environ, {"LO_TKRON_EPILOGUE": "1"}):
        y2 = host(K.matvec(desc, rhs))
    assert np.allclose(y, y2, rtol=1e-6, atol=1e-6)


def _no_closure_paths():
    """Patches that fail the test if an engine takes the closure (LO_OP_CALLBACK) path or the generic pivoted Cholesky
    instead of the descriptor."""
    def boom(*a, **k):
        raise AssertionError("the closure path ran instead of the Toeplitz Kronecker kind")

    return (mock.patch.object(K, "_wrap_closure", side_effect=boom),
            mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom))


def _solver_settings():
    return (settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.max_cholesky_size(0),
            settings.min_preconditioning_size(100))


@pytest.mark.parametrize("p", list(CASES))
def test_solve_runs_the_native_kind_and_matches_the_golden(p):
    A = AddedDiagLinearOperator(kron(p), DiagLinearOperator(dev(X[p + "_d"])))
    assert A._kernel_descriptor().kind == KIND
    p1, p2 = _no_closure_paths()
    s1, s2, s3, s4 = _solver_settings()
    with p1, p2, s1, s2, s3, s4:
        K._hip.prof_enable(True)
        x = A.solve(dev(X[p + "_rhs"]))  # pivoted Cholesky (descriptor rows), preconditioner, CG
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
    assert "ski_grid_mv" in prof and "pc_update" in prof, prof.keys()
    ref = G[p + "_solve"]
    assert np.allclose(host(x), ref, rtol=1e-3, atol=1e-3 * np.abs(ref).max())


def test_lanczos_and_minres_run_on_the_descriptor():
    A = AddedDiagLinearOperator(kron("g2"), DiagLinearOperator(dev(X["g2_d"])))
    desc = A._kernel_descriptor()
    A64 = host(A.to_dense()).astype(np.float64)
    p1, p2 = _no_closure_paths()
    with p1, p2:
        R = A.root_decomposition(method="lanczos").root.to_dense()
        r = K.minres_solve(desc, dev(X["g2_rhs"]), torch.zeros(1, device="cuda"), max_iter=400, tolerance=1e-5)
    assert torch.isfinite(R).all()
    b = X["g2_rhs"].astype(np.float64)
    res = np.linalg.norm(A64 @ host(r.x[0]).astype(np.float64) - b, axis=-2) / np.linalg.norm(b, axis=-2)
    assert res.max() <= 1e-4, res  # the solver's own tolerance plus one decade for the fp32 products


def test_pivoted_cholesky_against_golden():
    A = kron("pc")
    p1, p2 = _no_closure_paths()
    with p1, p2:
        L, piv = pivoted_cholesky(A, PC_RANK, error_tol=1e-6, return_pivots=True)
        L2, piv2 = pivoted_cholesky(A, PC_RANK, error_tol=1e-6, return_pivots=True)
    assert np.array_equal(host(piv), G["pc_piv"])
    assert np.abs(host(L) - G["pc_L"]).max() <= 3e-3 * np.abs(G["pc_L"]).max()
    assert np.array_equal(host(L), host(L2)) and np.array_equal(host(piv), host(piv2))


def test_inv_quad_logdet_forward_and_backward_against_golden():
    Z = dev(X["g2_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    dd, c1, c2 = (dev(X[k]).clone().requires_grad_(True) for k in ("g2_d", "g2_c1", "g2_c2"))
    s1, s2, s3, s4 = _solver_settings()
    with s1, s2, s3, s4, settings.num_trace_samples(6):
        A = Probed(kron("g2", [c1, c2]), DiagLinearOperator(dd))
        assert A._kernel_descriptor().kind == KIND
        iq, ld = A.inv_quad_logdet(dev(X["g2_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
    for name, got in (("iq", iq), ("ld", ld), ("dd", dd.grad), ("dc1", c1.grad), ("dc2", c2.grad)):
        ref = G["iql_" + name]
        print(f"inv_quad_logdet {name}: max err / max |ref| = {np.abs(host(got) - ref).max() / np.abs(ref).max():.3e}")
    assert close(iq, G["iql_iq"]) and close(ld, G["iql_ld"])
    assert close(dd.grad, G["iql_dd"]) and close(c1.grad, G["iql_dc1"]) and close(c2.grad, G["iql_dc2"])


@pytest.mark.parametrize("grid", [(1025, 2), (3, 2, 3, 2)])
def test_beyond_the_limits_the_torch_closed_form_serves(grid):
    cols = [column(3950 + k, 1, m, ls=0.3) for k, m in enumerate(grid)]
    A = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(dev(t)) for t in cols])
    assert A._kernel_descriptor() is None
    M = int(np.prod(grid))
    u = rng(3960).standard_normal((1, M, 2)).astype(np.float32)
    v = rng(3961).standard_normal((1, M, 2)).astype(np.float32)
    with mock.patch.object(K, "toeplitz_kron_bilinear", side_effect=AssertionError("native beyond its limits")):
        grads = A._bilinear_derivative(dev(u), dev(v))
    ref = grads64([t[0] for t in cols], u[0], v[0])
    for g, r in zip(grads, ref):
        assert np.linalg.norm(host(g)[0] - r) / np.linalg.norm(r) <= 1e-4
