"""Additive SKI on the MI355X: the kind LO_OP_SKI_SUM_DIAG and the two building blocks of csrc/lo_ski_sum.hip against the
float64 dense truth of the sparse form and the reference's goldens (tests/golden/g45_ski_sum_*.npz).

The bar of a product is BAR = 1e-4 per column, the project's fp32-against-fp64 bar (tests/test_gpu_block.py)."""
import ctypes as C
import functools
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ski_sum_cases as S  # noqa: E402

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.functions import pivoted_cholesky  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
    SumBatchLinearOperator, ToeplitzLinearOperator)
from linear_operator_amd.operators.added_diag_linear_operator import clear_preconditioner_memo  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1e-4
X = S.ski_sum_inputs()
KIND = _hip.LO_OP_SKI_SUM_DIAG
# (B, P, N, M, J) over B in {1, 2}, P in {1, 2, 3, 5}, N in {1, 257, 300}, M in {37, 64}, J in {4, 16}: B = 2 with
# P = 2, 3, 5 so that a swap of the b / p member indexing shows (members g = b P + p and g' = p B + b differ), N = 1
# and N no multiple of the block, both grid sizes and widths
COMBOS = [(1, 1, 1, 37, 4), (2, 3, 300, 64, 4), (1, 5, 257, 37, 16), (2, 2, 257, 64, 16), (2, 5, 300, 37, 4),
          (1, 2, 1, 64, 16), (2, 1, 257, 64, 4)]
COLUMNS = (1, 3, 17, 33)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def col_err(y, ref):
    y = np.asarray(y, np.float64)
    return (np.linalg.norm(y - ref, axis=-2) / np.linalg.norm(ref, axis=-2)).max()


@functools.lru_cache(maxsize=None)
def problem(combo, shared, oob):
    """(col, li, lv, ri, rv) as numpy, the float64 dense matrix, the diagonal d [B, N]; computed once per case."""
    B, P, N, M, J = combo
    col, li, lv, ri, rv = S.operator_inputs(5000 + 7 * sum(combo), B, P, N, M, J, shared=shared)
    if oob:  # indices outside [0, M): they contribute nothing and are never dereferenced
        r = np.random.default_rng(sum(combo))
        li = np.where(r.random(li.shape) < 0.15, r.choice([-1, -7, M, M + 5, 1 << 40], li.shape), li)
        ri = li if shared else np.where(r.random(ri.shape) < 0.15, r.choice([-1, M, M + 3, -(1 << 35)], ri.shape), ri)
    d = (0.1 + np.random.default_rng(N + P).random((B, N))).astype(np.float32)
    return col, li, lv, ri, rv, S.dense64(col, li, lv, ri, rv), d


def descriptor(col, li, lv, ri, rv, d=None, const=False):
    tl, tv = dev(li), dev(lv)
    tr, trv = (tl, tv) if (ri is li and rv is lv) else (dev(ri), dev(rv))
    return K.ski_sum_diag_descriptor(dev(col), tl, tv, tr, trv, None if d is None else dev(d), const)


def operator(col, li, lv, ri, rv):
    tl, tv = dev(li), dev(lv)
    tr, trv = (tl, tv) if (ri is li and rv is lv) else (dev(ri), dev(rv))
    return SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(dev(col)), tl, tv, tr, trv))


def diag_cases(d):
    """(d as the descriptor takes it, constant?, the diagonal as [B, N] float64) for the three diagonal modes."""
    return ((None, False, 0.0), (d, False, d.astype(np.float64)),
            (d[:, 0].copy(), True, np.repeat(d[:, :1].astype(np.float64), d.shape[1], 1)))


# ---- the product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=str)
def test_product_against_the_float64_truth(combo):
    B, P, N, M, J = combo
    worst = 0.0
    for shared in (False, True):
        for oob in (False, True):
            col, li, lv, ri, rv, dense, d = problem(combo, shared, oob)
            for c in COLUMNS:
                v = np.random.default_rng(c + N).standard_normal((B, N, c)).astype(np.float32)
                for dd, const, d64 in diag_cases(d):
                    ref = dense @ v.astype(np.float64) + (d64[..., None] * v if dd is not None else 0.0)
                    desc = descriptor(col, li, lv, ri, rv, dd, const)
                    assert desc is not None and desc.kind == KIND and desc.kernel_terms == P
                    err = col_err(host(K.matvec(desc, dev(v))), ref)
                    worst = max(worst, err)
                    assert err <= BAR, (combo, shared, oob, c, const, err)
    print(f"ski_sum {combo}: worst column error of lo_matvec_f32 {worst:.2e}")


@pytest.mark.parametrize("combo", [c for c in COMBOS if c[2] > 1], ids=str)
def test_operator_matmul_against_the_float64_truth(combo):
    """A._matmul of the class and of AddedDiag around it (whatever route the routing table sends them), both diagonal
    operators, distinct and shared interpolation sides."""
    B, P, N, M, J = combo
    for shared in (False, True):
        col, li, lv, ri, rv, dense, d = problem(combo, shared, False)
        A = operator(col, li, lv, ri, rv)
        assert A._kernel_descriptor().kind == KIND
        for c in COLUMNS:
            v = np.random.default_rng(c).standard_normal((B, N, c)).astype(np.float32)
            ref = dense @ v.astype(np.float64)
            assert col_err(host(A._matmul(dev(v))), ref) <= BAR
            full = AddedDiagLinearOperator(A, DiagLinearOperator(dev(d)))
            assert full._kernel_descriptor().kind == KIND and full._kernel_descriptor().diag_mode == _hip.LO_DIAG_FULL
            assert col_err(host(full._matmul(dev(v))), ref + d.astype(np.float64)[..., None] * v) <= BAR
            cd = ConstantDiagLinearOperator(dev(d[:, :1].copy()), N)
            const = AddedDiagLinearOperator(A, cd)
            assert const._kernel_descriptor().diag_mode == _hip.LO_DIAG_CONST
            assert col_err(host(const._matmul(dev(v))), ref + d.astype(np.float64)[:, :1, None] * v) <= BAR


@pytest.mark.parametrize("p", ["a", "b"])
def test_product_against_the_goldens(p):
    g = golden("g45_ski_sum_" + p)
    arrays = [X[f"{p}_{k}"] for k in ("col", "li", "lv", "ri", "rv")]
    A, desc = operator(*arrays), descriptor(*arrays)
    for c in S.COLS:
        v = dev(X[f"{p}_rhs{c}"])
        assert np.allclose(host(K.matvec(desc, v)), g[f"matmul{c}"], rtol=1e-4, atol=1e-5), c
        assert np.allclose(host(A._matmul(v)), g[f"matmul{c}"], rtol=1e-4, atol=1e-5), c
        assert np.allclose(host(A.matmul(v)), g[f"matmul{c}"], rtol=1e-4, atol=1e-5), c


def test_the_kind_runs_its_own_kernels():
    arrays = [X[f"a_{k}"] for k in ("col", "li", "lv", "ri", "rv")]
    desc = descriptor(*arrays, X["a_d"])
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        K.matvec(desc, dev(X["a_rhs3"]))
        torch.cuda.synchronize()
        prof = _hip.prof_report()
    finally:
        _hip.prof_enable(False)
    assert {"ski_interp_t", "ski_toeplitz_mv", "ski_interp_sum"} <= set(prof), prof.keys()
    assert "ski_interp" not in prof  # (the single-term gather is not what sums the terms)


# ---- bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [(2, 1, 257, 64, 4), (1, 1, 300, 37, 16), (1, 1, 1, 37, 4)], ids=str)
def test_one_term_has_the_bits_of_the_ski_kind(combo):
    B, P, N, M, J = combo
    for shared in (False, True):
        col, li, lv, ri, rv, _, d = problem(combo, shared, True)
        for dd, const, _ in diag_cases(d):
            one = descriptor(col, li, lv, ri, rv, dd, const)
            tl, tv = dev(li[:, 0]), dev(lv[:, 0])
            tr, trv = (tl, tv) if shared else (dev(ri[:, 0]), dev(rv[:, 0]))
            ski = K.ski_diag_descriptor(dev(col[:, 0]), tl, tv, tr, trv, None if dd is None else dev(dd), const)
            for c in COLUMNS:
                v = dev(np.random.default_rng(c).standard_normal((B, N, c)).astype(np.float32))
                assert torch.equal(K.matvec(one, v), K.matvec(ski, v)), (combo, shared, const, c)


def test_one_term_pivoted_cholesky_has_the_bits_of_the_ski_kind():
    """The two kinds search their pivots on different diagonals: LO_OP_SKI_DIAG on the reference's APPROXIMATE diagonal of
    an InterpolatedLinearOperator, (W_l sqrt(t0)) o (W_r sqrt(t0)), this kind on the exact one, which is what the
    reference's SumBatch hands its pivot search.  The rows are the same code.  Bit equality of the whole factor therefore
    holds exactly where the two diagonals round alike: one interpolation point per row (J = 1) on a column with
    t[0] = 1, where both are lv[i] rv[i].  That is the case compared here; with J > 1 the diagonals differ by design
    (shown at the end), and the goldens of both kinds pin each to its reference."""
    B, N, M = 2, 300, 64
    g = np.linspace(0.0, 1.0, M)
    col = np.stack([np.exp(-0.5 * (g / ls) ** 2) for ls in (0.07, 0.11)]).astype(np.float32)
    assert (col[:, 0] == 1.0).all()
    li, lv = S.interp(5100, B, N, M, 1)
    one = descriptor(col[:, None], li[:, None], lv[:, None], li[:, None], lv[:, None])
    tl, tv = dev(li), dev(lv)
    ski = K.ski_diag_descriptor(dev(col), tl, tv, tl, tv, None)
    L1, p1 = K.pivoted_cholesky(one, 10, 1e-6)
    L2, p2 = K.pivoted_cholesky(ski, 10, 1e-6)
    assert L1.shape[-1] == 10 and torch.equal(p1, p2) and torch.equal(L1, L2)
    # J = 4: the exact and the approximate diagonal are different numbers
    A = operator(X["pa_col"][:, :1], X["pa_li"][:, :1], X["pa_lv"][:, :1], X["pa_li"][:, :1], X["pa_lv"][:, :1])
    assert not torch.allclose(A._diagonal(), A.base_linear_op._approx_diagonal().sum(-2), rtol=1e-3)


def test_two_calls_give_equal_bits_and_a_canary_behind_y_survives():
    combo = (2, 3, 300, 64, 4)
    B, P, N, M, J = combo
    col, li, lv, ri, rv, _, d = problem(combo, False, True)
    desc = descriptor(col, li, lv, ri, rv, d)
    lib = _hip.load()
    for c in COLUMNS:
        v = dev(np.random.default_rng(c).standard_normal((B, N, c)).astype(np.float32))
        y1 = K.matvec(desc, v)
        buf = torch.full((B * N * c + 64,), -7.0, device="cuda")
        s = desc.c_struct()
        need = lib.lo_matvec_workspace_bytes(C.byref(s), c)
        ws = _hip.workspace(need, v.device)
        rc = lib.lo_matvec_f32(C.byref(s), _hip.ptr(v), _hip.ptr(buf), c, _hip.ptr(ws), need, _hip.stream_ptr(v.device))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(buf[:B * N * c].reshape(B, N, c), y1), c
        assert bool((buf[B * N * c:] == -7.0).all()), c
    L1, p1 = K.pivoted_cholesky(descriptor(X["pa_col"], X["pa_li"], X["pa_lv"], X["pa_li"], X["pa_lv"]), 10, 1e-6)
    L2, p2 = K.pivoted_cholesky(descriptor(X["pa_col"], X["pa_li"], X["pa_lv"], X["pa_li"], X["pa_lv"]), 10, 1e-6)
    assert torch.equal(L1, L2) and torch.equal(p1, p2)


def test_a_kept_right_plan_gives_the_bits_of_the_plan_built_per_call():
    for combo in ((2, 3, 300, 64, 4), (1, 5, 257, 37, 16)):
        B, P, N, M, J = combo
        col, li, lv, ri, rv, _, d = problem(combo, False, True)
        own = descriptor(col, li, lv, ri, rv, d)
        kept = descriptor(col, li, lv, ri, rv, d)
        kept.interp_plan = K.interp_plan_build(dev(ri).reshape(B * P, N, J), M)
        lib = _hip.load()
        for c in COLUMNS:
            v = dev(np.random.default_rng(c).standard_normal((B, N, c)).astype(np.float32))
            assert torch.equal(K.matvec(own, v), K.matvec(kept, v))
            a, b = own.c_struct(), kept.c_struct()
            assert lib.lo_matvec_workspace_bytes(C.byref(b), c) < lib.lo_matvec_workspace_bytes(C.byref(a), c)
        # the operator's lowering keeps the copy across calls (the memo over the B P members)
        A = operator(col, li, lv, ri, rv)
        d1, d2 = A._kernel_descriptor(), A._kernel_descriptor()
        assert d1.interp_plan is not None and d1.interp_plan.data_ptr() == d2.interp_plan.data_ptr()
        v = dev(np.random.default_rng(9).standard_normal((B, N, 3)).astype(np.float32))
        assert torch.equal(K.matvec(d1, v), K.matvec(descriptor(col, li, lv, ri, rv), v))


# ---- building blocks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", [(2, 3, 300, 64, 4), (1, 5, 257, 37, 16), (2, 2, 1, 37, 4)], ids=str)
def test_building_blocks(combo):
    B, P, N, M, J = combo
    col, li, lv, ri, rv, dense, d = problem(combo, False, True)
    plan = K.interp_plan_build(dev(ri).reshape(B * P, N, J), M)
    for c in COLUMNS:
        rng = np.random.default_rng(c)
        v = rng.standard_normal((B, N, c)).astype(np.float32)
        # W_p^T v from one v
        ref_u = np.zeros((B, P, M, c))
        ok = (ri >= 0) & (ri < M)
        contrib = rv.astype(np.float64)[..., None] * v.astype(np.float64)[:, None, :, None, :]  # [B, P, N, J, c]
        for b in range(B):
            for p in range(P):
                np.add.at(ref_u[b, p], ri[b, p][ok[b, p]], contrib[b, p][ok[b, p]])
        u = K.interp_t_bcast(plan, dev(rv), dev(v), M)
        nz = np.linalg.norm(ref_u, axis=-2) > 0
        err = np.linalg.norm(host(u) - ref_u, axis=-2)[nz] / np.linalg.norm(ref_u, axis=-2)[nz]
        assert u.shape == (B, P, M, c) and err.max() <= BAR
        # the bits of the single-member kernel on a [P, N, c] copy of v
        vcopy = dev(v)[:, None].expand(B, P, N, c).reshape(B * P, N, c).contiguous()
        assert torch.equal(u.reshape(B * P, M, c), K.interp_t_planned(plan, dev(rv).reshape(B * P, N, J), vcopy, M))
        # sum_p W_p w_p + d o v
        w = rng.standard_normal((B, P, M, c)).astype(np.float32)
        okl = (li >= 0) & (li < M)
        bi, pi = np.arange(B)[:, None, None, None], np.arange(P)[None, :, None, None]
        gathered = w.astype(np.float64)[bi, pi, np.clip(li, 0, M - 1)]  # [B, P, N, J, c]
        ref_y = (gathered * (lv.astype(np.float64) * okl)[..., None]).sum((1, 3))
        for dd, const, d64 in diag_cases(d):
            y = K.interp_sum(dev(li), dev(lv), dev(w), None if dd is None else dev(dd), None if dd is None else dev(v))
            want = ref_y + (d64[..., None] * v if dd is not None else 0.0)
            assert col_err(host(y), want) <= BAR, (c, const)
        # the kind is the composition of the blocks, bit for bit
        tu = K.toeplitz_mv(dev(col).reshape(B * P, M), u.reshape(B * P, M, c)).reshape(B, P, M, c)
        y = K.interp_sum(dev(li), dev(lv), tu, dev(d), dev(v))
        assert torch.equal(y, K.matvec(descriptor(col, li, lv, ri, rv, d), dev(v)))


# ---- workspace and refusals ------------------------------------------------------------------------------------------------
def test_workspace_bound_and_refusals_launch_nothing():
    combo = (2, 3, 300, 64, 4)
    B, P, N, M, J = combo
    col, li, lv, ri, rv, _, d = problem(combo, False, False)
    desc = descriptor(col, li, lv, ri, rv, d)
    lib = _hip.load()
    c = 3
    v = dev(np.random.default_rng(1).standard_normal((B, N, c)).astype(np.float32))
    y = torch.full((B, N, c), -7.0, device="cuda")
    st = _hip.stream_ptr(v.device)
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(C.byref(s), c)
    ws = _hip.workspace(need, v.device)
    run = lambda s_, nbytes=need: lib.lo_matvec_f32(C.byref(s_), _hip.ptr(v), _hip.ptr(y), c, _hip.ptr(ws), nbytes, st)  # noqa: E731
    L, perm = torch.empty(B, 10, N, device="cuda"), torch.empty(B, N, dtype=torch.int64, device="cuda")
    rank = C.c_int32(0)
    pc_need = lib.lo_pivoted_cholesky_workspace_bytes(C.byref(s), 10)
    pc_ws = _hip.workspace(pc_need, v.device)
    bad, unsup = -1, _hip.LO_ERR_UNSUPPORTED

    def mutated(field, val):
        s_ = desc.c_struct()
        if field in ("left_idx", "left_vals", "right_idx", "right_vals"):
            setattr(s_._interp_keepalive, field, val)
        elif field == "interp":
            s_.terms = None
        else:
            setattr(s_, field, val)
        return s_

    table = [("A0", None, bad), ("interp", None, bad), ("left_idx", None, bad), ("left_vals", None, bad),
             ("right_idx", None, bad), ("right_vals", None, bad), ("nterms", 0, bad), ("n2", 0, bad),
             ("nterms", _hip.LO_SKI_SUM_MAX_TERMS + 1, unsup), ("R", _hip.LO_TOEPLITZ_MAX_M + 1, unsup),
             ("N", 1 << 29, unsup)]
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        for field, val, rc in table:
            assert run(mutated(field, val)) == rc, (field, val)
            s_ = mutated(field, val)
            s_.diag_mode, s_.d = 0, None
            assert lib.lo_pivoted_cholesky_f32(C.byref(s_), 10, 1e-3, _hip.ptr(L), _hip.ptr(perm), C.byref(rank),
                                               _hip.ptr(pc_ws), pc_need, st) == rc, (field, val)
        assert run(s, need - 1) == -3  # LO_ERR_WORKSPACE one byte under the query
        # the solvers refuse the same descriptors through the same plan
        over = descriptor(col, li, lv, ri, rv, d)
        over.kernel_terms = _hip.LO_SKI_SUM_MAX_TERMS + 1
        for call in (lambda: K.matvec(over, v), lambda: K.cg_solve(over, v, max_iter=5),
                     lambda: K.lanczos_tridiag(over, v, 4),
                     lambda: K.minres_solve(over, v, torch.zeros(1, device="cuda"), max_iter=5),
                     lambda: K.pivoted_cholesky(over.without_diag(), 10)):
            with pytest.raises(_hip.HipExtensionError):
                call()
        # entry points that do not lower the kind
        s64 = desc.c_struct()
        assert lib.lo_matvec_f64(C.byref(s64), _hip.ptr(v), _hip.ptr(y), c, _hip.ptr(ws), need, st) == unsup
        assert not K.solve_fused_supported(desc, 1, 15)
        assert K.masked_descriptor(desc.without_diag(), torch.arange(8, device="cuda")) is None
        assert K.block_matvec(desc.without_diag(), _hip.LO_BLOCK_SUM, 2, v[:1]) is None
        torch.cuda.synchronize()
        assert _hip.prof_report() == {}, "a refusal launched a kernel"
    finally:
        _hip.prof_enable(False)
    assert bool((y == -7.0).all())
    assert run(s) == 0  # success at the query
    torch.cuda.synchronize()
    assert torch.equal(y, K.matvec(desc, v))


# ---- pivoted Cholesky -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", ["a", "b"])
def test_pivoted_cholesky_against_the_golden(p):
    """Pivots equal to the reference's; the factor within 1e-4 of the golden relative to its largest entry (the factor
    holds exact zeros: above the pivots, and where the Schur complement vanishes)."""
    g = golden("g45_ski_sum_pivchol_" + p)
    A = operator(X[f"p{p}_col"], X[f"p{p}_li"], X[f"p{p}_lv"], X[f"p{p}_li"], X[f"p{p}_lv"])
    assert A._kernel_descriptor().kind == KIND
    with mock.patch.object(K, "pivoted_cholesky_generic", side_effect=AssertionError("the generic row access ran")):
        L, piv = pivoted_cholesky(A, S.PIVCHOL_RANK, error_tol=S.PIVCHOL_TOL, return_pivots=True)
    m = g["L"].shape[-1]
    assert L.shape[-1] == m and np.array_equal(host(piv)[..., :m], g["piv"][..., :m])
    err = np.abs(host(L) - g["L"]).max() / np.abs(g["L"]).max()
    print(f"ski_sum pivoted Cholesky {p}: factor error relative to its largest entry {err:.2e}")
    assert err <= 1e-4
    # the diagonal the pivots are searched on is SumBatch._diagonal(), the exact one: the first pivot is its argmax and
    # L[q0, 0] its square root; the entries of column 0 are row q0 of the matrix over that square root
    diag = host(A._diagonal()).astype(np.float64)
    assert np.allclose(diag, g["diag"], rtol=1e-4, atol=1e-5)
    q0 = host(piv)[:, 0]
    assert np.array_equal(q0, diag.argmax(-1))
    l0 = host(L)[..., 0]
    assert np.allclose(l0[np.arange(len(q0)), q0], np.sqrt(diag.max(-1)), rtol=1e-6)
    dense = S.dense64(X[f"p{p}_col"], X[f"p{p}_li"], X[f"p{p}_lv"], X[f"p{p}_li"], X[f"p{p}_lv"])
    rows = dense[np.arange(len(q0)), q0] / np.sqrt(diag.max(-1))[:, None]
    assert np.abs(l0 - rows).max() <= 1e-5 * np.abs(rows).max()


# ---- public API --------------------------------------------------------------------------------------------------------------
def big(grad=False):
    col, dd, lv, li = dev(X["big_col"]), dev(X["big_d"]), dev(X["big_lv"]), dev(X["big_li"])
    if grad:
        col, dd, lvl, lvr = (t.clone().requires_grad_(True) for t in (col, dd, lv, lv))
    else:
        lvl = lvr = lv
    base = SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lvl, li, lvr))
    return base, col, dd, lvl, lvr


def close(a, b, rel=3e-3):  # the bar of g29_ski_solve's gradients (tests/test_gpu_ski.py)
    a, b = host(a), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * np.abs(b).max()


def test_public_api_meets_the_goldens_without_a_python_call_per_product_or_pivot():
    g, gg = golden("g45_ski_sum_solve"), golden("g45_ski_sum_grads")
    Z = dev(X["big_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    rhs = dev(X["big_rhs"])
    calls = []

    def counted(cls, name):
        real = getattr(cls, name)

        def wrapper(self, *a, **k):
            calls.append((cls.__name__, name))
            return real(self, *a, **k)

        return mock.patch.object(cls, name, wrapper)

    def boom(*a, **k):
        raise AssertionError("the closure route ran instead of the kind")

    clear_preconditioner_memo()
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        base, col, dd, _, _ = big()
        A = AddedDiagLinearOperator(base, DiagLinearOperator(dd))
        assert A._kernel_descriptor().kind == KIND
        with counted(SumBatchLinearOperator, "_matmul"), counted(InterpolatedLinearOperator, "_matmul"), \
                counted(SumBatchLinearOperator, "_get_rows"), counted(InterpolatedLinearOperator, "_get_rows"), \
                counted(SumBatchLinearOperator, "_get_indices"), counted(InterpolatedLinearOperator, "_get_indices"), \
                mock.patch.object(K, "_wrap_closure", side_effect=boom), \
                mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom):
            _hip.prof_enable(True)
            try:
                _hip.prof_report()
                x = A.solve(rhs)  # pivoted Cholesky (descriptor rows), preconditioner, CG
                torch.cuda.synchronize()
                prof = _hip.prof_report()
            finally:
                _hip.prof_enable(False)
            assert not calls, f"Python calls during the solve and the preconditioner build: {sorted(set(calls))}"
            assert {"ski_interp_sum", "pc_update"} <= set(prof), prof.keys()
            assert np.allclose(host(x), g["solve"], rtol=1e-4, atol=1e-4 * np.abs(g["solve"]).max())
            baseg, colg, ddg, lvl, lvr = big(grad=True)
            Ag = Probed(baseg, DiagLinearOperator(ddg))
            iq, ld = Ag.inv_quad_logdet(rhs, logdet=True)
            assert not calls, f"Python calls during inv_quad_logdet: {sorted(set(calls))}"
            R = A.root_decomposition(method="lanczos").root.to_dense()  # Lanczos
            sq = A.sqrt_inv_matmul(rhs)  # MINRES
            assert not calls, f"Python calls during Lanczos / MINRES: {sorted(set(calls))}"
        assert np.allclose(host(iq), g["iq"], rtol=1e-4, atol=0)
        assert np.allclose(host(ld), g["ld"], rtol=1e-4, atol=2048 * 1.2e-7 * 10.0)
        (iq.sum() + ld.sum()).backward()
    assert close(colg.grad, g["dcol"]) and close(ddg.grad, g["dd"])
    assert close(lvl.grad[..., ::S.GRAD_ROW_STEP, :], gg["dlv"]) and close(lvr.grad[..., ::S.GRAD_ROW_STEP, :], gg["drv"])
    # Lanczos root: R R^T agrees with A on the span of R
    assert torch.isfinite(R).all() and R.shape[:-1] == (2, 2048)
    q = torch.linalg.qr(R)[0]
    assert close(R @ (R.mT @ q), host(A._matmul(q.contiguous())), 1e-3)
    # MINRES: the same contour-integral quadrature through the closure route (the descriptor forced to None).  Both are
    # fp32 MINRES runs on the same shifted systems that stop at the same relative residual (settings.minres_tolerance,
    # 1e-4); the CG solve of this operator, stopped at 1e-5, meets its golden at 1e-4, a factor 10 for the conditioning,
    # and the same factor is allowed to each of the two runs here: 2 * 10 * 1e-4 relative to the largest entry
    class Closure(AddedDiagLinearOperator):
        def _kernel_descriptor(self, batch_shape=None):
            return None

    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        sq_ref = Closure(base, DiagLinearOperator(dd)).sqrt_inv_matmul(rhs)
    err = (sq - sq_ref).abs().max().item() / sq_ref.abs().max().item()
    print(f"ski_sum sqrt_inv_matmul: the kind against the closure route {err:.2e}")
    assert torch.isfinite(sq).all() and err <= 2e-3


# ---- outside the gate ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["float64", "rectangular", "grid above the limit"])
def test_operators_outside_the_gate_take_the_composition(case):
    g = golden("g45_ski_sum_a")
    arrays = [X[f"a_{k}"] for k in ("col", "li", "lv", "ri", "rv")]
    assert operator(*arrays)._kernel_descriptor().kind == KIND  # inside the gate, for comparison
    col, li, lv, ri, rv = (dev(a) for a in arrays)
    if case == "float64":
        A = SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col.double()), li, lv.double(), ri,
                                                              rv.double()))
        assert A._kernel_descriptor() is None
        for c in S.COLS:
            assert np.allclose(host(A._matmul(dev(X[f"a_rhs{c}"]).double())), g[f"matmul{c}"], rtol=1e-4, atol=1e-5)
    elif case == "rectangular":  # the first 200 rows of the left side
        A = SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li[..., :200, :].contiguous(),
                                                              lv[..., :200, :].contiguous(), ri, rv))
        assert A.shape == (2, 200, 300) and A._kernel_descriptor() is None
        for c in S.COLS:
            assert np.allclose(host(A._matmul(dev(X[f"a_rhs{c}"]))), g[f"matmul{c}"][:, :200], rtol=1e-4, atol=1e-5)
    else:  # M above LO_TOEPLITZ_MAX_M: the goldens' operator on a grid padded with points no row touches
        M = _hip.LO_TOEPLITZ_MAX_M + 1
        wide = torch.zeros(2, 3, M, device="cuda")
        wide[..., :64] = col
        A = SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(wide), li, lv, ri, rv))
        assert A._kernel_descriptor() is None
        assert np.allclose(host(A._matmul(dev(X["a_rhs3"]))), g["matmul3"], rtol=1e-4, atol=1e-5)
