"""Edge cases of the 1-D Toeplitz / SKI kernels (csrc/lo_ski.hip), shared by tests/test_ski_edges_cpu.py (the cases' own
preconditions, no GPU) and tests/test_gpu_ski_edges.py (the kernels against the references below).  Everything here is
numpy: restatements of the launch arithmetic (`tz_split`, `bil_split`, the column chunks, the scatter switch, the grid
caps, the byte layout of an interpolation plan), the case tables, the inputs and the references.  Not a test module.

Every kernel of the file is sums of products.  The inputs are integers from {+-1, +-2, +-3} (never 0) and weights from
{1/4, 1/2, 3/4, 1}, so every product and every partial sum is a multiple of 1/16 (1/4 with one weight, 1 with none)
below 2^24 units: exactly representable in float32 in any summation order, with or without fmaf.  The kernels must
return the reference bit for bit; a dropped, doubled or mis-indexed term moves the result by at least one unit."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski import interp as uniform_interp  # noqa: E402

# ---- restated from csrc/lo_ski.hip -------------------------------------------------------------------------------------
THREADS = 256                  # kThreads, kTzRows, kTzK, kBilI
TZ_MAX_COLS = 32               # kTzMaxCols
TZ_CB = (1, 2, 4, 8, 16, 24, 32)   # the instantiations of k_tz_mv
ELEM_CAP = 8192 * THREADS      # grid_for: elements of one pass of an element-per-thread kernel (2,097,152)
WAVE_CAP = 32768 * 4           # waves of one pass of k_csr_sort and k_interp_t_wave (131,072)
SCATTER_LANE_FROM = 8          # interp_scatter_bcast: a wave per output below, a lane per output from here on


def ceil_div(a, b):
    return -(-a // b)


def align256(n):
    return ceil_div(n, 256) * 256


def tz_split(B, M):
    """(RB, KS, kchunk, length of the last k slice) of the Toeplitz product."""
    RB = ceil_div(M, THREADS)
    ks = ceil_div(512, B * RB)
    KS = max(1, min(ks, ceil_div(M, THREADS)))
    kchunk = ceil_div(ceil_div(M, KS), THREADS) * THREADS
    KS = ceil_div(M, kchunk)
    return RB, KS, kchunk, M - (KS - 1) * kchunk


def bil_split(B, M):
    """(LB, KI, ichunk, length of the last i slice) of the lag correlation."""
    LB = ceil_div(M, THREADS)
    ki = max(1, min(ceil_div(512, B * LB), ceil_div(M, THREADS)))
    ichunk = ceil_div(ceil_div(M, ki), THREADS) * THREADS
    KI = ceil_div(M, ichunk)
    return LB, KI, ichunk, M - (KI - 1) * ichunk


def toeplitz_workspace_bytes(B, M, c):
    """lo_toeplitz_workspace_bytes: the split-k partials or the split-i partials, whichever is larger."""
    return max(align256(4 * tz_split(B, M)[1] * B * M * c), align256(4 * bil_split(B, M)[1] * B * M)) + 256


def column_chunks(c):
    """[(col0, cc, CB)]: the launches of k_tz_mv for c columns."""
    out = []
    for col0 in range(0, c, TZ_MAX_COLS):
        cc = min(TZ_MAX_COLS, c - col0)
        out.append((col0, cc, next(cb for cb in TZ_CB if cc <= cb)))
    return out


def scatter_mode(c):
    return "wave" if c < SCATTER_LANE_FROM else "lane"


def plan_layout(B, N, J, M):
    """({name: (byte offset, int32 count)}, end of the last array): csr_layout's four takes, each aligned to 256."""
    out, off = {}, 0
    for name, n in (("ptr", B * (M + 1)), ("cur", B * (M + 1)), ("tmp", B * N * J), ("ids", B * N * J)):
        off = align256(off)
        out[name] = (off, n)
        off += 4 * n
    return out, off


def plan_bytes(B, N, J, M):
    return plan_layout(B, N, J, M)[1] + 256


def plan_arrays(plan_bytes_host, B, N, J, M):
    """The int32 arrays of a plan read back from the device: ptr, cur [B, M + 1]; tmp, ids [B, N J]."""
    lay, _ = plan_layout(B, N, J, M)
    raw = np.asarray(plan_bytes_host, np.uint8)
    arr = {k: raw[o:o + 4 * n].view(np.int32) for k, (o, n) in lay.items()}
    return {k: a.reshape(B, M + 1 if k in ("ptr", "cur") else N * J) for k, a in arr.items()}


def wraps(B, M, N, J, c, S=1):
    """Which grid-stride loops make a second pass at a shape."""
    return {"k_csr_count": B * N * J > ELEM_CAP, "k_csr_fill": B * N * J > ELEM_CAP,
            "k_interp_vgrad": B * N * J > ELEM_CAP, "k_csr_sort": B * M > WAVE_CAP,
            "k_interp_t_wave": scatter_mode(c) == "wave" and B * M * c > WAVE_CAP,
            "k_interp_t_lane": scatter_mode(c) == "lane" and B * M * c > ELEM_CAP,
            "k_interp": B * N * c > ELEM_CAP, "k_tz_reduce": B * M * c > ELEM_CAP}


# ---- inputs ------------------------------------------------------------------------------------------------------------
LIMIT = 1 << 24   # units below which every float32 sum is exact
QUARTERS = np.array([0.25, 0.5, 0.75, 1.0], np.float32)
INTS = np.array([-3, -2, -1, 1, 2, 3], np.float32)


def rng(*key):
    return np.random.Generator(np.random.PCG64([4200, *key]))


def ints(r, shape):
    return r.choice(INTS, size=shape)


def quarters(r, shape):
    return r.choice(QUARTERS, size=shape)


def lag_column(r, B, M):
    """t [B, M] from INTS with t[k] != t[k - 1] for every k: a lag read one off is a different number wherever it is."""
    t = ints(r, (B, M))
    for k in range(1, M):
        same = t[:, k] == t[:, k - 1]
        t[same, k] = -t[same, k]
    return t


def const_diag(B):
    """One integer of INTS per member, neighbours different: what LO_DIAG_CONST reads at dd[b]."""
    b = np.arange(B)
    return ((b % 3 + 1) * np.where(b % 2, -1, 1)).astype(np.float32)


# ---- the Toeplitz product ------------------------------------------------------------------------------------------------
# (B, M): what tz_split / bil_split make of each is asserted in tests/test_ski_edges_cpu.py
TZ_SHAPES = ((1, 1), (1, 2), (1, 255), (1, 256), (1, 257), (1, 513), (1, 517), (40, 1030), (64, 1030), (171, 517))
TZ_COLS_ONE = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 40, 64, 65)   # B = 1: every CB, every cc < CB, three chunks
TZ_COLS_BATCHED = (1, 3, 33)
BIL_S = (1, 2, 5)


def tz_cols(B):
    return TZ_COLS_ONE if B == 1 else TZ_COLS_BATCHED


def toeplitz_dense(t):
    """T[i, k] = t[|i - k|] of one member in float64."""
    m = np.arange(t.shape[-1])
    return t.astype(np.float64)[np.abs(m[:, None] - m[None, :])]


def toeplitz_ref(t, u):
    """T u per member through the dense matrix (one member's at a time): t [B, M], u [B, M, c] -> float64."""
    return np.stack([toeplitz_dense(t[b]) @ u[b].astype(np.float64) for b in range(t.shape[0])])


@functools.lru_cache(maxsize=None)
def tz_case(B, M, c):
    """(t [B, M], u [B, M, c], d [B, M], T u in float64) of a product case; built once."""
    r = rng(1, B, M, c)
    t, u, d = lag_column(r, B, M), ints(r, (B, M, c)), ints(r, (B, M))
    ref = toeplitz_ref(t, u)
    for a in (t, u, d, ref):
        a.setflags(write=False)
    return t, u, d, ref


def diag_term(d, v, mode):
    """d o v for mode "none" / "full" (d [B, rows]) / "const" (d [B])."""
    if mode == "none":
        return 0.0
    d = d.astype(np.float64)
    return (d[:, :, None] if mode == "full" else d[:, None, None]) * v.astype(np.float64)


# ---- the lag correlation -------------------------------------------------------------------------------------------------
def bil_ref_definition(u, v):
    """g [B, M] as tests/test_gpu_ski.py::test_backward_kernels_against_fp64 writes it: g_0 = sum u o v,
    g_k = sum_s sum_i u[i] v[i + k] + u[i + k] v[i]."""
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    B, M, _ = u.shape
    ref = np.zeros((B, M))
    ref[:, 0] = (u64 * v64).sum((1, 2))
    for k in range(1, M):
        ref[:, k] = (u64[:, :-k] * v64[:, k:]).sum((1, 2)) + (u64[:, k:] * v64[:, :-k]).sum((1, 2))
    return ref


def bil_ref(u, v):
    """The same sums taken as the diagonals of C = U V^T per member (integers in float64: exact in any order)."""
    B, M, _ = u.shape
    m = np.arange(M)
    lag = (m[None, :] - m[:, None] + M - 1).ravel()
    out = np.zeros((B, M))
    for b in range(B):
        diag = np.bincount(lag, weights=(u[b].astype(np.float64) @ v[b].astype(np.float64).T).ravel(), minlength=2 * M - 1)
        out[b] = diag[M - 1:] + diag[M - 1::-1]
        out[b, 0] = diag[M - 1]
    return out


@functools.lru_cache(maxsize=None)
def bil_case(B, M, S):
    r = rng(2, B, M, S)
    u, v = ints(r, (B, M, S)), ints(r, (B, M, S))
    ref = bil_ref(u, v)
    for a in (u, v, ref):
        a.setflags(write=False)
    return u, v, ref


# ---- interpolation -------------------------------------------------------------------------------------------------------
INTERP_C = (1, 7, 8, 9)                  # both sides of the wave / lane switch
VGRAD_S = (1, 5)
BCAST_P, BCAST_C = 3, (7, 8)

# (name, pattern, B, M, N, J)
INTERP_CASES = (
    ("uniform-M1000-J4", "uniform", 3, 1000, 300, 4),
    ("uniform-M256-J16", "uniform", 1, 256, 100, 16),
    ("uniform-M255-J1", "uniform", 3, 255, 64, 1),
    ("clustered-N1", "clustered", 1, 256, 1, 4),      # segments of exactly 1 entry
    ("clustered-N64", "clustered", 3, 255, 64, 4),    # of 64: one full trip of the wave kernel's lanes
    ("clustered-N65", "clustered", 1, 1000, 65, 16),  # of 65: a second trip of one lane
    ("clustered-N200", "clustered", 3, 256, 200, 4),  # of 200 = 3 * 64 + 8
    ("clustered-M1", "clustered", 1, 1, 200, 1),      # a grid of one point
    ("empty", "empty", 3, 1000, 3, 4),                # M >> N J: nearly every segment has beg == end
    ("duplicate-M255", "duplicate", 3, 255, 100, 4),
    ("duplicate-M1", "duplicate", 1, 1, 5, 4),
    ("duplicate-J16", "duplicate", 1, 256, 50, 16),
    ("outside-M1000", "outside", 3, 1000, 200, 4),
    ("outside-M255-J16", "outside", 1, 255, 64, 16),
    ("outside-M256-J1", "outside", 3, 256, 100, 1),
    ("outside-M1", "outside", 1, 1, 10, 4),
)
INTERP_BY_NAME = {row[0]: row for row in INTERP_CASES}
CSR_CASES = tuple(n for n, p, *_ in INTERP_CASES if p in ("clustered", "duplicate", "outside"))
WRAP = ("wrap", "uniform", 9, 16384, 15000, 16)
WRAP_C = (1, 16)


def outside_values(M):
    return (-1, M, M + 5, -(1 << 40))


def clustered_points(r, M, J):
    """J distinct grid points, the two ends of the grid among them (J = 1: any one point)."""
    assert M >= J
    if J == 1:
        return r.integers(0, M, size=1)
    return np.concatenate(([0, M - 1], 1 + r.permutation(M - 2)[:J - 2]))


def make_indices(pattern, r, B, M, N, J):
    """idx int64 [B, N, J] of a pattern."""
    if pattern in ("uniform", "empty", "duplicate", "outside"):
        if M > J + 1:
            idx, _ = uniform_interp(int(r.integers(1 << 30)), B, N, M, J)   # the generator of tests/test_gpu_ski.py
        else:
            idx = r.integers(0, M, size=(B, N, J))
    if pattern == "clustered":   # all N rows of a member on the same J distinct points
        idx = np.repeat(np.stack([clustered_points(r, M, J) for _ in range(B)])[:, None, :], N, axis=1)
    if pattern == "duplicate" and J > 1:   # the same grid point twice (J >= 4: three times) within a row
        idx[..., 1] = idx[..., 0]
        if J >= 4:
            idx[..., 3] = idx[..., 0]
    if pattern == "outside":   # a quarter of the entries outside [0, M), all four values in turn; row 0: nothing else
        out = np.array(outside_values(M), np.int64)
        flat = idx.reshape(-1)
        pos = np.flatnonzero(r.random(flat.size) < 0.25)
        flat[pos] = out[np.arange(pos.size) % 4]
        idx[:, 0, :] = out[np.arange(J) % 4]
    return np.ascontiguousarray(idx.astype(np.int64))


@functools.lru_cache(maxsize=None)
def interp_case(name, members=None):
    """(idx int64, vals fp32 [B, N, J]) of a case; `members`: another member count than the table's (for the P terms of
    interp_t_bcast)."""
    _, pattern, B, M, N, J = WRAP if name == "wrap" else INTERP_BY_NAME[name]
    B = members or B
    r = rng(3, sum(map(ord, name)), B)
    idx = make_indices(pattern, r, B, M, N, J)
    vals = quarters(r, (B, N, J))
    idx.setflags(write=False)
    vals.setflags(write=False)
    return idx, vals


def case_shape(name):
    return (WRAP if name == "wrap" else INTERP_BY_NAME[name])[2:]


def operand(name, what, rows, c, members=None):
    """An integer operand [B, rows, c] of a case (`what` names it: "u", "v", "lv", "R")."""
    B = members or case_shape(name)[0]
    return ints(rng(4, sum(map(ord, name + what)), B, rows, c), (B, rows, c))


def in_range(idx, M):
    return (idx >= 0) & (idx < M)


def w_ref(idx, vals, u):
    """W u in float64, a member at a time; entries outside [0, M) are dropped.  -> [B, N, c]."""
    B, N, J = idx.shape
    M = u.shape[1]
    out = np.empty((B, N, u.shape[2]))
    for b in range(B):
        ok = in_range(idx[b], M)
        w = np.where(ok, vals[b], 0).astype(np.float64)
        out[b] = np.einsum("njc,nj->nc", u[b].astype(np.float64)[np.where(ok, idx[b], 0)], w)
    return out


def wt_ref(idx, vals, v, M):
    """W^T v in float64 (np.add.at), a member at a time; entries outside [0, M) are dropped.  -> [B, M, c]."""
    B, N, J = idx.shape
    out = np.zeros((B, M, v.shape[2]))
    for b in range(B):
        ok = in_range(idx[b], M).reshape(-1)
        contrib = (vals[b].astype(np.float64)[:, :, None] * v[b].astype(np.float64)[:, None, :]).reshape(N * J, -1)
        np.add.at(out[b], idx[b].reshape(-1)[ok], contrib[ok])
    return out


def vgrad_ref(idx, lv, R):
    """g[n, j] = sum_s lv[n, s] R[idx[n, j], s] in float64, 0 for an entry outside [0, M).  -> [B, N, J]."""
    B, N, J = idx.shape
    M = R.shape[1]
    out = np.empty((B, N, J))
    for b in range(B):
        ok = in_range(idx[b], M)
        g = np.einsum("ns,njs->nj", lv[b].astype(np.float64), R[b].astype(np.float64)[np.where(ok, idx[b], 0)])
        out[b] = np.where(ok, g, 0.0)
    return out


def csr_ref(idx, M):
    """(ptr [B, M + 1], [ids of member b]): the exclusive cumulative count of in-range indices per grid point, and every
    point's entries in ascending entry order."""
    B, N, J = idx.shape
    ptr = np.zeros((B, M + 1), np.int64)
    ids = []
    for b in range(B):
        flat = idx[b].reshape(-1)
        keep = np.flatnonzero(in_range(flat, M))
        ptr[b, 1:] = np.cumsum(np.bincount(flat[keep], minlength=M))
        ids.append(keep[np.argsort(flat[keep], kind="stable")])
    return ptr, ids


def segment_lengths(idx, M):
    ptr, _ = csr_ref(idx, M)
    return np.diff(ptr, axis=1)


# ---- the SKI kind end to end: y = W_l T W_r^T v + d o v ----------------------------------------------------------------
SKI_SHAPES = ((1, 257, 300, 4), (3, 517, 400, 4))   # (B, M, N, J)
SKI_C = (1, 8, 33)
DIAG_MODES = ("none", "full", "const")


@functools.lru_cache(maxsize=None)
def ski_case(B, M, N, J, outside):
    """{t, li, lv, ri, rv, d_full, d_const}: both sides' weights; `outside`: a quarter of the indices of either side
    outside [0, M)."""
    r = rng(5, B, M, N, J, int(outside))
    pattern = "outside" if outside else "uniform"
    out = {"t": lag_column(r, B, M), "li": make_indices(pattern, r, B, M, N, J), "lv": quarters(r, (B, N, J)),
           "ri": make_indices(pattern, r, B, M, N, J), "rv": quarters(r, (B, N, J)), "d_full": ints(r, (B, N)),
           "d_const": const_diag(B)}
    for a in out.values():
        a.setflags(write=False)
    return out


def ski_ref(t, li, lv, ri, rv, v, d, mode, absolute=False):
    """W_l (T (W_r^T v)) + d o v in float64; `absolute`: the same chain over absolute values, the sum of the absolute
    terms that bounds every partial sum."""
    if absolute:
        t, lv, rv, v = np.abs(t), np.abs(lv), np.abs(rv), np.abs(v)
        d = None if d is None else np.abs(d)
    M = t.shape[1]
    return w_ref(li, lv, toeplitz_ref(t, wt_ref(ri, rv, v, M))) + diag_term(d, v, mode)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def exact(got, ref):
    """Whether the float32 array `got` IS `ref` (float64): equal element for element after casting ref to float32, which
    must lose nothing."""
    ref = np.asarray(ref, np.float64)
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref), "the reference is not representable in float32"
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    return got.shape == ref.shape and np.array_equal(got, r32)


def mismatches(got, ref, limit=8):
    """Where and by how much `got` differs from `ref`, for a failing assertion's message."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return f"shape {got.shape} against {ref.shape}"
    bad = np.argwhere(~(got == ref))
    rows = [f"{tuple(int(x) for x in i)}: {float(got[tuple(i)])!r} != {float(ref[tuple(i)])!r}" for i in bad[:limit]]
    return f"{len(bad)} of {got.size} differ; first: " + "; ".join(rows)
