"""Edge cases of the SKI grid kind (csrc/lo_ski_grid.hip, the grid branches of csrc/lo_pivchol.hip), shared by
tests/test_ski_grid_edges_cpu.py (the cases' own preconditions, no GPU) and tests/test_gpu_ski_grid_edges.py (the
kernels against the references below).  Everything here is numpy: a table of product shapes with the branch of
`grid_axis` each is meant to reach, a restatement of that selection rule, the fp64 grid product, and the pivoted
Cholesky recurrence of W_l K W_r^T in fp64 and in float32.  Not a test module."""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import column, rng  # noqa: E402
from make_golden_ski_grid import PC_RANK, grid_interp, kron_dense64, w_dense64  # noqa: E402

# ---- the product: which kernel an axis goes to -----------------------------------------------------------------------
THREADS = 256  # kThreads
TILE = 64      # kGridTile: the j tile and the s tile of k_grid_axis_inner
STAGE = 4096   # kGridStage: floats of a line chunk in k_grid_axis_line

# (grid, c, B, label per axis).  The labels are what expected_route() must return: a shape that stops reaching its
# branch (the selection rule changed, or the arithmetic below was wrong) fails tests/test_ski_grid_edges_cpu.py.
PRODUCT_CASES = (
    # axis 2: inner = 5, LS = 5120, two chunks of the line (819 and 205 rows), 20 workgroups per line, a second member
    ((3, 1024), 5, 2, ("inner2", "line_chunked(819,205)")),
    # axis 2: the widest line (inner = 63): 16 chunks of 65 rows, the last of 25
    ((2, 1000), 63, 1, ("inner8[rows,s,j]", "line_chunked(65,25)")),
    # axis 2: inner = 64, the other side of the boundary: k_grid_axis_inner with exactly one full s tile
    ((2, 1000), 64, 1, ("inner8[rows,j]", "inner2")),
    # axis 3: LS = 8, 30 lines per workgroup with three members: a workgroup must not mix members
    ((6, 5, 4), 2, 3, ("line_shared(1)", "line_shared(6)", "line_shared(30)")),
    # axis 3: LS = 6, outer = 65: the divisor search starts at 42 and must fall to 13
    ((13, 5, 3), 2, 2, ("line_split(2)", "line_shared(1)", "line_shared(13)")),
    # axis 1: 8 rows per thread with M = 40 < 64 (one zero-padded j tile, rows 40..63 guarded); axis 2: M = 70 (a ragged
    # 32-row tile, a ragged j tile) and inner = 268 (a ragged s tile)
    ((40, 70, 67), 4, 1, ("inner8[rows,s,j]", "inner8[rows,s,j]", "line_split(2)")),
    # axis 1: 8 rows per thread at LO_SKI_GRID_MAX_AXIS, the window at its full size
    ((1024, 64), 16, 1, ("inner8", "line_split(4)")),
    # axis 1: 2 rows per thread at the maximal axis
    ((1024, 64), 1, 1, ("inner2", "line_shared(4)")),
    # axis 1: k_grid_axis_inner with M_k = 1
    ((1, 70), 1, 2, ("inner2", "line_shared(1)")),
    # axis 2: LS = 3, lpb = 7 = outer, the smallest shared line
    ((7, 3), 1, 1, ("line_shared(1)", "line_shared(7)")),
)

# every kind of label expected_route() can return (numbers dropped, one entry per ragged tail of the 8-row kernel)
ROUTE_KINDS = frozenset({"inner8", "inner8+rows", "inner8+s", "inner8+j", "inner2", "line_shared", "line_split",
                         "line_chunked"})


def shared_lines_start(Mk, inner, outer):
    """Where the divisor search of a shared line starts: min(256 / LS, outer)."""
    return min(THREADS // (Mk * inner), outer)


def expected_route(grid, c, B):
    """The kernel and tiling `grid_axis` (csrc/lo_ski_grid.hip) selects for every axis of (T_1 (x) .. (x) T_D) u,
    u [B, M, c], restated from the source: one label per axis.  Not a correctness oracle: it only says which branch a
    shape exercises."""
    M = math.prod(grid)
    labels, outer = [], 1
    for Mk in grid:
        inner = M // (outer * Mk) * c
        lines = B * outer
        if inner >= TILE:
            stiles = -(-inner // TILE)
            if lines * stiles * ((Mk + 31) // 32) >= 512:
                tails = [name for name, ragged in (("rows", Mk % 32), ("s", inner % TILE), ("j", Mk % TILE)) if ragged]
                labels.append("inner8" + (f"[{','.join(tails)}]" if tails else ""))
            else:
                labels.append("inner2")
        else:
            LS = Mk * inner
            if LS >= THREADS:
                bpl = -(-LS // THREADS)
                jc = min(Mk, STAGE // inner)
                labels.append(f"line_chunked({jc},{Mk - (Mk - 1) // jc * jc})" if jc < Mk else f"line_split({bpl})")
            else:
                lpb = shared_lines_start(Mk, inner, outer)
                while outer % lpb:
                    lpb -= 1
                labels.append(f"line_shared({lpb})")
        outer *= Mk
    return tuple(labels)


def route_kinds(label):
    """The entries of ROUTE_KINDS a label stands for."""
    name = label.split("(")[0].split("[")[0]
    if "[" not in label:
        return {name}
    return {f"{name}+{t}" for t in label[label.index("[") + 1:-1].split(",")}


def product_inputs(grid, c, B):
    """(columns [B, M_k] per axis, u [B, M, c]) of a product case: per-member columns as in
    tests/test_gpu_ski_grid.py, so that the members differ; u standard normal."""
    cols = [column(3700 + k, B, m, ls=0.2) * (1.0 + 0.1 * rng(3710 + k).standard_normal((B, m))).astype(np.float32)
            for k, m in enumerate(grid)]
    M = math.prod(grid)
    u = rng(3720 + M + c).standard_normal((B, M, c)).astype(np.float32)
    return cols, u


def kron_apply64(cols, u):
    """(T_1 (x) .. (x) T_D) u in fp64 for one member: the dense symmetric Toeplitz matrix of every factor applied along
    its axis of u [M_1, .., M_D, c] (the Kronecker product itself is not formed)."""
    y = u.astype(np.float64).reshape(*[t.shape[-1] for t in cols], -1)
    for k, t in enumerate(cols):
        m = t.shape[-1]
        Tk = t.astype(np.float64)[np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])]
        y = np.moveaxis(np.tensordot(Tk, y, axes=(1, k)), 0, k)
    return y.reshape(u.shape)


def col_err(y, ref):
    y = np.asarray(y, np.float64)
    return (np.linalg.norm(y - ref, axis=-2) / np.linalg.norm(ref, axis=-2)).max()


# ---- the pivoted Cholesky of W_l K W_r^T ----------------------------------------------------------------------------
def _w_dense_dropping64(idx, vals, M):
    """One member's W [N, M] in fp64; weights whose index is outside [0, M) are dropped."""
    ok = (idx >= 0) & (idx < M)
    return w_dense64(np.where(ok, idx, 0), np.where(ok, vals, np.float32(0.0)), M)


def pivchol64(cols, li, lv, ri, rv, rank):
    """The reference recurrence (functions/_pivoted_cholesky.py:14-105) of W_l K W_r^T for one member in fp64: pivots
    are chosen on the approximate diagonal t0 rowsum(W_l) rowsum(W_r), downdated; rows come from the true matrix.
    cols[k] [M_k]; li, ri int64 and lv, rv fp32 [N, J].  Returns (pivots [rank], L [N, rank], the relative gap between
    the two largest remaining diagonal entries at every step [rank], the smallest remaining diagonal entry seen)."""
    M = math.prod(t.shape[-1] for t in cols)
    Wl, Wr = _w_dense_dropping64(li, lv, M), _w_dense_dropping64(ri, rv, M)
    A = Wl @ kron_dense64(cols) @ Wr.T
    t0 = np.prod([float(t[0]) for t in cols])
    diag = t0 * Wl.sum(-1) * Wr.sum(-1)
    N = A.shape[0]
    perm = np.arange(N)
    L = np.zeros((rank, N))
    gaps, low = [], diag.min()
    for m in range(rank):
        rem = np.sort(diag[perm[m:]])[::-1]
        gaps.append((rem[0] - rem[1]) / rem[0])
        j = m + int(np.argmax(diag[perm[m:]]))
        perm[[m, j]] = perm[[j, m]]
        pi = perm[m]
        L[m, pi] = np.sqrt(diag[pi])
        rest = perm[m + 1:]
        row = (A[pi, rest] - L[:m, pi] @ L[:m, rest]) / L[m, pi]
        L[m, rest] = row
        diag[rest] -= row ** 2
        low = min(low, diag[rest].min())
    return perm[:rank].copy(), L.T.copy(), np.array(gaps), float(low)


def pivchol32(cols, li, lv, ri, rv, rank):
    """The same recurrence in numpy float32 in the operation order documented in csrc/lo_pivchol.hip: every product
    rounded on its own, every sum sequential.
      t0      = t_1[0] (t_2[0] t_3[0]), s = sqrt(t0)
      diag_i  = (sum_j s lv[i, j]) (sum_j s rv[i, j]), j ascending
      row_i   = sum_b sum_a base(li[p, a], ri[i, b]) (lv[p, a] rv[i, b]), b outer and a inner, with
                base(g, h) = (t_1[|g_1 - h_1|] t_2[|g_2 - h_2|]) t_3[|g_3 - h_3|] (0 when g or h is outside the grid)
      L[m, i] = (row_i - sum_{j < m} L[j, p] L[j, i]) / sqrt(diag_p), j ascending;  diag_i -= L[m, i]^2
    A reference of its own, not the code under test.  Returns (pivots [rank], L [N, rank])."""
    f = np.float32
    cols = [np.asarray(t, f) for t in cols]
    grid = [t.shape[-1] for t in cols]
    M, D = math.prod(grid), len(grid)
    lv, rv = np.asarray(lv, f), np.asarray(rv, f)
    N, J = li.shape
    t0 = cols[-1][0]
    for k in range(D - 2, -1, -1):
        t0 = f(cols[k][0] * t0)
    s = np.sqrt(f(t0))
    lok, rok = (li >= 0) & (li < M), (ri >= 0) & (ri < M)
    lt, rt = np.where(lok, s * lv, f(0)), np.where(rok, s * rv, f(0))
    diag = np.add.accumulate(lt, axis=1, dtype=f)[:, -1] * np.add.accumulate(rt, axis=1, dtype=f)[:, -1]
    assert diag.dtype == f

    def split(g):  # the grid coordinates of an index, trailing axis fastest
        out = []
        for m in grid[::-1]:
            out.append(g % m)
            g = g // m
        return out[::-1]

    rq = split(np.where(rok, ri, 0))  # D x [N, J]
    perm = np.arange(N)
    L = np.zeros((rank, N), f)
    for m in range(rank):
        j = m + int(np.argmax(diag[perm[m:]]))
        perm[[m, j]] = perm[[j, m]]
        p = perm[m]
        piv = np.sqrt(diag[p])
        L[m, p] = piv
        pq = split(np.where(lok[p], li[p], 0))  # D x [J]
        base = None  # [N, J (b), J (a)]
        for k in range(D):
            fk = cols[k][np.abs(rq[k][:, :, None] - pq[k][None, None, :])]
            base = fk if base is None else base * fk
        base = np.where(rok[:, :, None] & lok[p][None, None, :], base, f(0))
        terms = base * (lv[p][None, None, :] * rv[:, :, None])
        assert terms.dtype == f
        row = np.add.accumulate(terms.reshape(N, J * J), axis=1, dtype=f)[:, -1]
        if m > 0:
            prods = L[:m, p][:, None] * L[:m]  # [m, N]
            row = row - np.add.accumulate(prods, axis=0, dtype=f)[-1]
        v = row / piv
        rest = perm[m + 1:]
        L[m, rest] = v[rest]
        diag[rest] = diag[rest] - v[rest] * v[rest]
    return perm[:rank].copy(), L.T.copy()


def member_columns(seed, B, grid, ls):
    """Columns [B, M_k] per axis whose members differ in shape, not only in scale: member b has the length scale
    ls[b] (every member stays positive definite)."""
    return [np.stack([column(seed + 10 * b + k, 1, m, ls=ls[b])[0] for b in range(B)]) for k, m in enumerate(grid)]


G3, G2 = (6, 5, 7), (12, 16)
# The seeds below were picked on the CPU so that at every pivot step of every member the two largest remaining entries
# of the fp64 diagonal are at least PC_GAP apart, the remaining diagonal stays positive and pivchol32 takes pivchol64's
# pivots (tests/test_ski_grid_edges_cpu.py asserts all three).
SEED_SHARED, SEED_MEMBERS, SEED_SEPARATE = 3800, 3823, 3840
# (member, row, slot, value) written into the indices of the out-of-grid case; M = 210.  Row 0 of the list is a pivot
# row of the fp64 recurrence, the last one is never a pivot (asserted on the CPU).
OOG_LEFT = ((0, 98, 5, 210), (0, 0, 40, -1))
OOG_RIGHT = ((0, 75, 17, -1), (0, 1, 63, 210))


@functools.lru_cache(maxsize=None)
def pivot_case(name):
    """(grid, cols, li, lv, ri, rv, shared): the inputs of a pivoted Cholesky case.  cols[k] is [M_k] (unbatched) or
    [B, M_k]; li, ri int64 and lv, rv fp32 [B, N, J]; `shared`: W_r is W_l (the same storage on the device)."""
    if name in ("g3_shared", "g3_out_of_grid"):
        cols = [column(SEED_SHARED + k, 1, m, ls=0.4)[0] for k, m in enumerate(G3)]
        li, lv = grid_interp(SEED_SHARED + 5, 1, 150, G3)
        if name == "g3_shared":
            return G3, cols, li, lv, li, lv, True
        li, ri, rv = li.copy(), li.copy(), lv.copy()
        for arr, edits in ((li, OOG_LEFT), (ri, OOG_RIGHT)):
            for b, row, slot, value in edits:
                arr[b, row, slot] = value
        return G3, cols, li, lv, ri, rv, False
    if name == "g3_members":
        cols = member_columns(SEED_MEMBERS, 3, G3, (0.3, 0.4, 0.5))
        li, lv = grid_interp(SEED_MEMBERS + 5, 3, 150, G3)
        return G3, cols, li, lv, li, lv, True
    if name == "g2_separate":
        cols = member_columns(SEED_SEPARATE, 2, G2, (0.25, 0.35))
        li, lv = grid_interp(SEED_SEPARATE + 5, 2, 192, G2)
        rv = (lv * (1.0 + 0.02 * rng(SEED_SEPARATE + 6).standard_normal(lv.shape))).astype(np.float32)
        return G2, cols, li, lv, li.copy(), rv, False
    raise KeyError(name)


PIVOT_CASES = ("g3_shared", "g3_members", "g2_separate", "g3_out_of_grid")


def member_cols(cols, b):
    return [t if t.ndim == 1 else t[b] for t in cols]


@functools.lru_cache(maxsize=None)
def pivot_reference64(name):
    """pivchol64 of every member of a case: a list of (pivots, L, gaps, smallest diagonal)."""
    _, cols, li, lv, ri, rv, _ = pivot_case(name)
    return [pivchol64(member_cols(cols, b), li[b], lv[b], ri[b], rv[b], PC_RANK) for b in range(li.shape[0])]


# max over the cases and members of max |L32 - L64| / max |L64| between pivchol32 and pivchol64 above, as printed by
# tests/test_ski_grid_edges_cpu.py::test_measured_rounding_level (which asserts that this is that figure, rounded up to
# two digits): the fp32 rounding level of the recurrence in the kernel's operation order at these shapes.
PC_ROUNDING = 1.5e-6  # (measured 1.424e-06: member 2 of g3_members)


# ---- the engines' operator: A = W (T_1 (x) T_2 (x) T_3) W^T + diag(d) on the 3-D grid, per-member columns -----------
@functools.lru_cache(maxsize=None)
def engine_case():
    """(grid, cols [2, M_k], li, lv [2, 150, 64], d [2, 150], A64 [2, 150, 150])."""
    B, N = 2, 150
    cols = member_columns(3860, B, G3, (0.3, 0.45))
    li, lv = grid_interp(3865, B, N, G3)
    d = (0.5 + 0.5 * rng(3866).random((B, N))).astype(np.float32)
    M = math.prod(G3)
    A = []
    for b in range(B):
        W = w_dense64(li[b], lv[b], M)
        A.append(W @ kron_dense64(member_cols(cols, b)) @ W.T + np.diag(d[b].astype(np.float64)))
    return G3, cols, li, lv, d, np.stack(A)
