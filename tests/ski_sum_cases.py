"""Inputs of the additive SKI tests (LO_OP_SKI_SUM_DIAG): one seeded function, shared by the golden generator
(tests/golden/make_golden_ski_sum.py), tests/test_ski_sum_cpu.py and tests/test_gpu_ski_sum.py.

An operator is SumBatch(Interpolated(Toeplitz(col [B, P, M]), li, lv, ri, rv [B, P, N, J])): P one-dimensional grids of
M points over the same N rows.  Every term has its own length scale and its own interpolation matrices (random positive
weights), so a mix-up of the terms, or of the b / p member indexing, changes the result."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import column, interp, rng  # noqa: E402

# (B, P, N, M, J) of the golden fixtures
SHAPES = {"a": (2, 3, 300, 64, 4), "b": (1, 5, 257, 37, 16), "big": (2, 3, 2048, 256, 4)}
COLS = (1, 3, 17)  # columns of the golden products
DENSE_ROWS = 32    # rows of to_dense() a fixture keeps (evenly spaced, first and last included): the fixture size limit
GRAD_ROW_STEP = 3  # the interpolation-value gradients of the solve fixture are kept at rows 0, 3, 6, ..
# seeds at which the generator's float64 pivot-gap assertion holds (another seed is picked there if it does not)
PIVCHOL_SEEDS = {"a": 4800, "b": 4900}
PIVCHOL_RANK, PIVCHOL_TOL = 10, 1e-6


def term_lengthscale(p, big=False):
    """Length scale of term p: all different (0.10, 0.13, 0.16, .. of the unit interval; the solve case shorter)."""
    return (0.04 if big else 0.10) + 0.03 * p


def operator_inputs(seed, B, P, N, M, J, shared=False, big=False):
    """col [B, P, M], (li, lv), (ri, rv) [B, P, N, J] -- the right side IS the left side when `shared`."""
    col = np.stack([column(seed + 10 * p, B, M, ls=term_lengthscale(p, big)) for p in range(P)], axis=1)
    left = [interp(seed + 10 * p + 1, B, N, M, J) for p in range(P)]
    li, lv = np.stack([t[0] for t in left], 1), np.stack([t[1] for t in left], 1)
    if shared:
        return col, li, lv, li, lv
    right = [interp(seed + 10 * p + 2, B, N, M, J) for p in range(P)]
    return col, li, lv, np.stack([t[0] for t in right], 1), np.stack([t[1] for t in right], 1)


def dense_rows(N):
    return np.unique(np.linspace(0, N - 1, DENSE_ROWS).round().astype(np.int64))


def ski_sum_inputs():
    """Every input of the fixtures, by name."""
    d = {}
    for k, name in enumerate(("a", "b")):
        B, P, N, M, J = SHAPES[name]
        seed = 4500 + 100 * k
        d[name + "_col"], d[name + "_li"], d[name + "_lv"], d[name + "_ri"], d[name + "_rv"] = operator_inputs(
            seed, B, P, N, M, J)
        for c in COLS:
            d[f"{name}_rhs{c}"] = rng(seed + 50 + c).standard_normal((B, N, c)).astype(np.float32)
        d[name + "_d"] = (0.05 + 0.1 * rng(seed + 90).random((B, N))).astype(np.float32)
        # the pivoted Cholesky factors a symmetric operator: the same shape with W_r = W_l
        d["p" + name + "_col"], d["p" + name + "_li"], d["p" + name + "_lv"], _, _ = operator_inputs(
            PIVCHOL_SEEDS[name], B, P, N, M, J, shared=True)
    B, P, N, M, J = SHAPES["big"]
    d["big_col"], d["big_li"], d["big_lv"], _, _ = operator_inputs(4700, B, P, N, M, J, shared=True, big=True)
    d["big_d"] = (0.05 + 0.1 * rng(4790).random((B, N))).astype(np.float32)
    d["big_rhs"] = rng(4791).standard_normal((B, N, 2)).astype(np.float32)
    d["big_Z"] = rng(4792).standard_normal((B, N, 6)).astype(np.float32)
    return d


# ---- float64 truth from the sparse form (no reference needed) ---------------------------------------------------------
def dense64(col, li, lv, ri, rv):
    """sum_p W_l,p T_p W_r,p^T as a float64 [B, N, N] matrix; index entries outside [0, M) contribute nothing."""
    B, P, M = col.shape
    N, J = li.shape[-2:]
    lag = np.abs(np.arange(M)[:, None] - np.arange(M)[None, :])
    out = np.zeros((B, N, N))
    for b in range(B):
        for p in range(P):
            T = col[b, p].astype(np.float64)[lag]
            Wl, Wr = np.zeros((N, M)), np.zeros((N, M))
            for W, idx, vals in ((Wl, li, lv), (Wr, ri, rv)):
                i, v = idx[b, p], vals[b, p].astype(np.float64)
                ok = (i >= 0) & (i < M)
                np.add.at(W, (np.repeat(np.arange(N), J)[ok.reshape(-1)], i.reshape(-1)[ok.reshape(-1)]),
                          v.reshape(-1)[ok.reshape(-1)])
            out[b] += Wl @ T @ Wr.T
    return out


def pivoted_cholesky64(K, rank):
    """Greedy pivoted Cholesky of one float64 PSD matrix: (pivots, the relative gap between the largest and the second
    largest remaining diagonal entry at every step)."""
    N = K.shape[0]
    diag = np.diag(K).copy()
    L = np.zeros((rank, N))
    perm = np.arange(N)
    piv, gaps = [], []
    for m in range(rank):
        rest = diag[perm[m:]]
        order = np.argsort(-rest, kind="stable")
        gaps.append((rest[order[0]] - rest[order[1]]) / rest[order[0]] if len(rest) > 1 else 1.0)
        j = m + order[0]
        perm[[m, j]] = perm[[j, m]]
        q = perm[m]
        piv.append(q)
        L[m, q] = np.sqrt(diag[q])
        tail = perm[m + 1:]
        L[m, tail] = (K[q, tail] - L[:m, q] @ L[:m, tail]) / L[m, q]
        diag[tail] -= L[m, tail] ** 2
    return np.array(piv), np.array(gaps)
