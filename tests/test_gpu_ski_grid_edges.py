"""The branches of the SKI grid kind that tests/test_gpu_ski_grid.py does not reach, on the MI355X: the grid product of
csrc/lo_ski_grid.hip on every path of `grid_axis` between guard bands, the pivoted Cholesky of the kind on a 3-D grid,
with per-member columns, separate right weights and out-of-grid indices, and CG / MINRES / Lanczos on a 3-D grid with
per-member columns -- all against plain fp64 references (tests/ski_grid_edge_cases.py; its preconditions are checked
without a GPU in tests/test_ski_grid_edges_cpu.py)."""
import ctypes as C
import math
from unittest import mock

import numpy as np
import pytest
import torch

import ski_grid_edge_cases as E
from make_golden_ski_grid import PC_RANK

from linear_operator_amd import kernels as K
from linear_operator_amd.functions import pivoted_cholesky
from linear_operator_amd.operators import (
    InterpolatedLinearOperator, KroneckerProductLinearOperator, ToeplitzLinearOperator)

pytestmark = pytest.mark.gpu
GUARD = 1024  # sentinel floats before and after u and y


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- 3a. the product between guard bands -----------------------------------------------------------------------------
def guarded(values, n):
    """A contiguous view of n floats in the middle of a 1-D buffer with GUARD sentinel floats (NaN) on either side,
    holding `values` (or the sentinel)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    if values is not None:
        buf[GUARD:GUARD + n] = values.reshape(-1)
    return buf, buf[GUARD:GUARD + n]


def guarded_product(t, grid, B, c, u):
    """lo_toeplitz_kron_mv_f32 the way K.toeplitz_kron_mv launches it, on guarded u and y.  Returns (y on the host,
    whether the four guard bands and u kept their bits)."""
    lib = K._hip.load()
    n = B * math.prod(grid) * c
    ubuf, uv = guarded(u, n)
    ybuf, yv = guarded(None, n)
    before = bits(ubuf).clone()
    m = (C.c_int64 * len(grid))(*grid)
    K._launch("lo_toeplitz_kron_mv_f32", ubuf.device, t, m, len(grid), B, uv.view(B, -1, c), c, yv.view(B, -1, c),
              ws_bytes=lib.lo_toeplitz_kron_workspace_bytes(m, len(grid), B, c))
    torch.cuda.synchronize()
    sentinel = bits(torch.full((GUARD,), float("nan"), dtype=torch.float32, device="cuda"))
    intact = (torch.equal(bits(ubuf), before) and torch.equal(bits(ybuf[:GUARD]), sentinel)
              and torch.equal(bits(ybuf[GUARD + n:]), sentinel))
    return host(yv).reshape(B, -1, c), intact


@pytest.mark.parametrize("grid,c,B,route", E.PRODUCT_CASES)
def test_grid_product_on_every_route_between_guard_bands(grid, c, B, route):
    cols, u = E.product_inputs(grid, c, B)
    ref = np.stack([E.kron_apply64([t[b] for t in cols], u[b]) for b in range(B)])
    t, ud = dev(np.concatenate(cols, -1)), dev(u)
    y1, intact1 = guarded_product(t, grid, B, c, ud)
    y2, intact2 = guarded_product(t, grid, B, c, ud)
    err = E.col_err(y1, ref)
    print(f"product {grid} c={c} B={B} [{' | '.join(route)}]: col_err {err:.3e}")
    assert intact1 and intact2, "the product wrote outside y or changed u"
    assert err <= 1e-4
    assert np.array_equal(y1.view(np.int32), y2.view(np.int32))


# ---- 3b. the pivoted Cholesky of the kind ----------------------------------------------------------------------------
# max |L - L64| <= PC_L_BOUND max |L64|: four times the fp32 rounding level of the recurrence measured on the CPU
# between pivchol32 and pivchol64 (E.PC_ROUNDING = 1.5e-6), the factor allowing for the kernel's sqrtf and division
# differing from numpy's by an ulp per step: 6e-6.
PC_L_BOUND = 4 * E.PC_ROUNDING
assert PC_L_BOUND == 6e-6


def pivot_descriptor(name):
    _, cols, li, lv, ri, rv, shared = E.pivot_case(name)
    li_d, lv_d = dev(li), dev(lv)
    ri_d, rv_d = (li_d, lv_d) if shared else (dev(ri), dev(rv))
    desc = K.ski_grid_diag_descriptor([dev(t) for t in cols], li_d, lv_d, ri_d, rv_d, None)
    assert desc.kind == K._hip.LO_OP_SKI_GRID_DIAG
    if not shared:
        assert desc.interp[2].data_ptr() != desc.interp[0].data_ptr()
        assert desc.interp[3].data_ptr() != desc.interp[1].data_ptr()
    return desc


@pytest.mark.parametrize("name", E.PIVOT_CASES)
def test_pivoted_cholesky_against_the_fp64_recurrence(name):
    desc = pivot_descriptor(name)
    L, perm = K.pivoted_cholesky(desc, PC_RANK, error_tol=1e-6)
    Ld, L, perm = L, host(L), host(perm)
    refs = E.pivot_reference64(name)
    assert L.shape == (len(refs), desc.N, PC_RANK) and perm.shape == (len(refs), desc.N)
    for b, (p64, L64, _, _) in enumerate(refs):
        err = np.abs(L[b] - L64).max() / np.abs(L64).max()
        print(f"pivoted Cholesky {name}[{b}]: max |L - L64| / max |L64| = {err:.3e} (bound {PC_L_BOUND:.1e})")
        assert np.array_equal(perm[b, :PC_RANK], p64), (b, perm[b, :PC_RANK], p64)
        assert sorted(perm[b].tolist()) == list(range(desc.N))
        assert err <= PC_L_BOUND, (b, err)
    L2, perm2 = K.pivoted_cholesky(desc, PC_RANK, error_tol=1e-6)
    assert same_bits(Ld, L2) and np.array_equal(perm, host(perm2))


def test_operator_level_pivoted_cholesky_is_the_descriptor_call():
    _, cols, li, lv, _, _, _ = E.pivot_case("g3_shared")
    L, perm = K.pivoted_cholesky(pivot_descriptor("g3_shared"), PC_RANK, error_tol=1e-6)
    base = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(dev(t)) for t in cols])
    li_d, lv_d = dev(li), dev(lv)

    def boom(*a, **k):
        raise AssertionError("the closure path ran instead of the SKI grid kind")

    with mock.patch.object(K, "_wrap_closure", side_effect=boom), \
            mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom):
        Lo, pivo = pivoted_cholesky(InterpolatedLinearOperator(base, li_d, lv_d, li_d, lv_d), PC_RANK, error_tol=1e-6,
                                    return_pivots=True)
    assert same_bits(Lo, L)
    assert np.array_equal(host(pivo), host(perm))


# ---- 3c. the engines on a 3-D grid with per-member columns -----------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    _, cols, li, lv, d, A64 = E.engine_case()
    li_d, lv_d = dev(li), dev(lv)
    desc = K.ski_grid_diag_descriptor([dev(t) for t in cols], li_d, lv_d, li_d, lv_d, dev(d))
    assert desc.kind == K._hip.LO_OP_SKI_GRID_DIAG and desc.B == 2 and desc.N == 150 and desc.grid == E.G3
    rhs = E.rng(3870).standard_normal((2, 150, 3)).astype(np.float32)
    return desc, A64, rhs


def residual64(A64, x, rhs):
    """|| A64 x - b || / || b || per member and column in fp64."""
    x, b = np.asarray(x, np.float64), rhs.astype(np.float64)
    return np.linalg.norm(A64 @ x - b, axis=-2) / np.linalg.norm(b, axis=-2)


def test_cg_on_a_3d_grid_with_per_member_columns(engine):
    desc, A64, rhs = engine
    r = [K.cg_solve(desc, dev(rhs), tolerance=1e-5, max_iter=400) for _ in range(2)]
    res = residual64(A64, host(r[0].x), rhs)
    print(f"CG: {r[0].iterations} iterations, fp64 residuals {res.max(-1)}")
    # the solver's own tolerance plus one decade for the rounding of the fp32 products
    assert res.max() <= 1e-4, res
    assert same_bits(r[0].x, r[1].x)


def test_minres_on_a_3d_grid_with_per_member_columns(engine):
    desc, A64, rhs = engine
    shifts = torch.zeros(1, device="cuda")
    r = [K.minres_solve(desc, dev(rhs), shifts, max_iter=400, tolerance=1e-5) for _ in range(2)]
    assert r[0].x.shape == (1, 2, 150, 3)
    res = residual64(A64, host(r[0].x[0]), rhs)
    print(f"MINRES: {r[0].iterations} iterations, fp64 residuals {res.max(-1)}")
    assert res.max() <= 1e-4, res
    assert same_bits(r[0].x, r[1].x)


def lanczos_error(A64, q, t):
    """max(|| Q^T A64 Q - T ||_max / || T ||_max, || Q^T Q - I ||_max) over the members, in fp64."""
    q, t = host(q).astype(np.float64), host(t).astype(np.float64)
    worst = 0.0
    for b in range(q.shape[0]):
        k = t.shape[-1]
        worst = max(worst, np.abs(q[b].T @ A64[b] @ q[b] - t[b]).max() / np.abs(t[b]).max(),
                    np.abs(q[b].T @ q[b] - np.eye(k)).max())
    return worst


def test_lanczos_on_a_3d_grid_with_per_member_columns(engine):
    desc, A64, _ = engine
    init = dev(E.rng(3871).standard_normal((2, 150, 1)).astype(np.float32))
    runs = [K.lanczos_tridiag(desc, init, 8) for _ in range(2)]
    q, t = runs[0]
    assert q.shape == (2, 150, 8) and t.shape == (2, 8, 8)
    # the yardstick: the same call on the dense kind (tested elsewhere, not the code under test) for the same matrix
    qd, td = K.lanczos_tridiag(K.dense_diag_descriptor(dev(A64.astype(np.float32)), None), init, 8)
    assert qd.shape == q.shape
    grid_err, dense_err = lanczos_error(A64, q, t), lanczos_error(A64, qd, td)
    print(f"Lanczos: grid kind {grid_err:.3e}, dense kind {dense_err:.3e}")
    assert grid_err <= 4 * dense_err, f"grid kind {grid_err:.3e} against 4 x {dense_err:.3e} of the dense kind"
    assert same_bits(q, runs[1][0]) and same_bits(t, runs[1][1])
