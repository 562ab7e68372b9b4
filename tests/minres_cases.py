"""Fixed-step iterates of the shifted MINRES engines (csrc/lo_minres.hip, csrc/lo_minres_f64.hip) as a table of tiny
cases, shared by tests/test_minres_cases_cpu.py (the conditions that make the comparison valid and the checker's teeth; no
GPU) and tests/test_gpu_minres_iterates.py (the kernels).  Everything here is numpy plus the oracle: the table, the seeded
operands, the references, the checker and the bounds.  Not a test module.

A MINRES run that converges hides most arithmetic faults: they cost iterations, not accuracy.  With `tolerance = 0` the
loop never stops and `max_iter = k - 2` gives exactly k iterations (`max_iter >= 0`: k >= 2), in the kernels and in
`oracle.lo_oracle.minres` alike, so the k-th iterate itself can be compared while it still moves by far more than the
bound per step.  References, all on the float32-rounded operands cast to float64 (both sides see the same operator):

    reference(name)   the oracle's run in float64: x_k [Q, B, N, c]
    krylov(name)      x_k = argmin ||b - (value K + sigma I) x|| over span{b, M b, .., M^(k-1) b}, from a twice
                      re-orthogonalised basis and a least-squares solve: what MINRES computes, without the recurrence
                      (unpreconditioned cases with k <= 12)
    oracle_f32(name)  the oracle's run in float32: the rounding a correct float32 run shows on the same inputs

`check(name, x)` returns, per (shift, member, column) and in float64,

    err     ||x - reference|| / ||reference||
    resid   | ||b - M x|| / ||b||  -  the same of the reference |     (M = value K + sigma I, or value K + sigma P with a
            preconditioner P: the shift enters the preconditioned recurrence, as in the reference implementation)
    zeros   the number of non-zero entries where the right-hand-side column is zero (must be 0)

Bounds (`bounds`): clamp(8 x the float32 oracle's own figure, 2e-6, 5e-4) for both figures.  8 x is the rule of
tests/lanczos_cases.py; 2e-6 = 8 x 2^-22 keeps a lucky float32 run of the oracle from setting a bound below rounding;
5e-4 is what tests/test_gpu_api.py asks of a converged MINRES run, and tests/test_minres_cases_cpu.py asserts that the
oracle's figure stays below 5e-4 / 8, so the cap only ever tightens the rule.  Float64 engine: 1e-10.  The bounds come
from the oracle, never from the library.

What the table leaves out, and why: one iteration (k = 1 needs max_iter = -1, which both entry points refuse; the k = 1
rows are kept as refusals) and a run beyond the Krylov space as a case of its own (N = 6, k = 9: after step N the iterate
has stopped moving, so no seed can meet the still-moving condition; the wrapper case `wrapper-cap-N6` runs those nine
steps and pins their count)."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lo_oracle as orc  # noqa: E402

f32, f64 = np.float32, np.float64
FACTOR, FLOOR, CAP = 8.0, 2e-6, 5e-4
F64_BOUND = 1e-10
KRYLOV_MAX_K = 12
MOVING = 100.0        # ||x_k - x_(k+-1)|| / ||x_k|| >= MOVING x bound
CONV_FLOOR = 1e-5     # relative floor of the bound on info.conv
MAX_COLS = 256        # kMaxCols of csrc/lo_internal.h
R = 8                 # rank of the low-rank operands

Case = namedtuple("Case", "name group kind B N c Q k per_member value tol max_iter precond dtype opts note seed")
# kind: lowrank | closure | dense | tensor | kron | toeplitz | sum  (float32: the descriptor handed to K.minres_solve;
#       "closure" the low-rank operator as an opaque callback, "tensor" the dense matrix handed to utils.minres)
#       f64dense | f64closure | f64lowrank | f64kron  (float64: minres_solve_f64's A=, matvec_closure=, desc=)
# k: iterations the run makes (max_iter = k - 2 when tol == 0).  precond: None | ("woodbury", rank) | "diag".
# opts: shifts= (array or callable(lam_max) -> array); d= "unit" [0.5, 1.5] | "wide" [dlo= 0.02, 1.5] with
#       ||C C^T|| < 0.1 (no outlying eigenvalues: about 0.8 per step, so the iterate still moves at step 20) |
#       "clusters"; cscale= the factor on C; rhs= "scales" | "zero"; refused= "iterations" | "columns" | "grid";
#       wrapper= "cap" | "broadcast"; kron=(n1, n2); seed= in place of the row's own; still_moving=False: exempt from
#       the still-moving condition (with the reason in the note)


def choose_split(B, N, min_rows=256, max_split=256):
    """(S, rows) of csrc/lo_vec.hip: choose_split, restated."""
    S = (1024 + B - 1) // B
    maxS = max(1, N // max(min_rows, 4))
    S = max(1, min(S, maxS))
    cap = 64
    while cap < max_split and (cap * 2) * (cap * 2) * 16 <= N:
        cap *= 2
    S = min(S, cap, max_split)
    rows = (N + S - 1) // S
    rows = (rows + 3) // 4 * 4
    return (N + rows - 1) // rows, rows


def dense_s_dot(B, N, c):
    """Partials per member the dense matvec writes (csrc/lo_dense.hip: dense_S_dot): one per 64-row tile on the matrix
    cores (c >= 2 and N >= 256), else one per workgroup of 16 .. 128 rows."""
    if c >= 2 and N >= 256:
        return (N + 63) // 64, "mfma"
    rows = 128
    while rows > 16 and B * ((N + rows - 1) // rows) < 1024:
        rows //= 2
    return (N + rows - 1) // rows, f"valu{rows}"


def kron_fused(n1, n2, c):
    """csrc/lo_kron.hip: kron_mfma_ok -- the Kronecker matvec writes its own partials (one per 128 x 128 tile)."""
    return c == 1 and n1 % 4 == 0 and n2 % 4 == 0 and n1 >= 64 and n2 >= 64


def s_dot(c):
    """(S_dot, does the kind's own matvec write the partials) of a float32 case."""
    S = choose_split(c.B, c.N)[0]
    if c.kind in ("dense", "tensor"):
        return dense_s_dot(c.B, c.N, c.c)[0], True
    if c.kind == "kron":
        n1, n2 = c.opts["kron"]
        fused = kron_fused(n1, n2, c.c)
        return (((n1 + 127) // 128) * ((n2 + 127) // 128) if fused else S), fused
    return S, c.kind == "lowrank"


def expected_vec_dot_part(c):
    """Launches of the shared epilogue k_dot_part one call makes: rhs . rhs, z_1 . z_1 (or, with a closure as the
    preconditioner, z . P^-1 z at the start and per iteration; the Woodbury kernels write their own partials), and
    q . K q per iteration for a kind whose matvec does not write them."""
    n = {None: 2, "diag": 2 + c.k}.get(c.precond, 1)
    return n + (0 if s_dot(c)[1] else c.k)


SH2 = (0.0, 0.7)
SH_SLOW = (0.0, 0.03)  # with d = "wide": both systems converge slowly


def _table():
    t = []

    def add(name, group, kind, B, N, c, k, shifts=SH2, per_member=False, value=None, tol=0.0, max_iter=None,
            precond=None, dtype="f32", note="", **opts):
        sh = shifts if callable(shifts) else np.asarray(shifts, dtype=f64)
        Q = opts.pop("Q", None) or (sh.shape[0] if not callable(sh) else 2)
        opts["shifts"] = sh
        t.append(Case(name, group, kind, B, N, c, Q, k, per_member, value, tol, k - 2 if max_iter is None else max_iter,
                      precond, dtype, opts, note, opts.pop("seed", 8000 + 10 * len(t))))

    # ---- slices: the multi-slice sums and the short last slice
    for N in (3, 6, 255, 260, 517, 1027, 1030):
        for k in (1, 2, 3):
            add(f"slices-N{N}-k{k}", "slices", "lowrank", 2, N, 3, k, **({"refused": "iterations"} if k == 1 else {}))
    add("slices-N6-k6", "slices", "lowrank", 2, 6, 3, 6, cscale=3.0, seed=8141,
        note="k = N: the Krylov space is the whole space (C C^T three times as strong, so that the sixth step still moves)")
    for k in (9, 10, 11):
        add(f"slices-N517-k{k}", "slices", "lowrank", 2, 517, 3, k, shifts=SH_SLOW, d="wide",
            note="the every-10th reduction pass runs (k >= 10) and stops nothing")
    # ---- columns: the thread map col = t % c, slot = t / c, nrs = 256 / c
    for c in (1, 2, 4, 5, 64, 85, 86, 128, 129, 255, 256):
        add(f"columns-c{c}", "columns", "lowrank", 2, 517, c, 3, note="low-rank descriptor (refuses no column count)")
    add("columns-c257", "columns", "lowrank", 2, 517, 257, 3, refused="columns")
    # ---- shifts
    add("shifts-Q1-shared", "shifts", "lowrank", 2, 517, 3, 3, shifts=(0.3,))
    add("shifts-Q1-member", "shifts", "lowrank", 2, 517, 3, 3, shifts=((0.3, 0.9),), per_member=True)
    add("shifts-Q5-member-B3", "shifts", "lowrank", 3, 517, 3, 3, shifts=0.1 * (1 + np.arange(15.0)).reshape(5, 3),
        per_member=True, note="15 distinct values")
    add("shifts-Q15-shared", "shifts", "lowrank", 2, 517, 3, 3, shifts=np.linspace(0.05, 3.0, 15))
    add("shifts-value-1", "shifts", "lowrank", 2, 517, 3, 3, shifts=lambda lam: np.ceil(lam) + np.array([1.0, 10.0]),
        value=-1.0, note="-K + sigma I with sigma above lambda_max: the form contour_integral_quad solves")
    add("shifts-value2.5", "shifts", "lowrank", 2, 517, 3, 3, value=2.5)
    add("shifts-indefinite", "shifts", "lowrank", 2, 517, 3, 3, shifts=(-1.15, 0.4), d="clusters", cscale=0.03,
        note="d in [0.5, 0.7] u [1.5, 1.7], ||C C^T|| < 0.1: K - 1.15 I has eigenvalues on both sides of 0, none within 0.3")
    # ---- right-hand sides (S = 2)
    add("rhs-scales", "rhs", "lowrank", 2, 517, 3, 3, rhs="scales", note="columns scaled by 1, 1e3, 1e-3")
    add("rhs-zero-column", "rhs", "lowrank", 2, 517, 3, 3, rhs="zero", note="last member, last column all zero")
    add("rhs-zero-column-tol1", "rhs", "lowrank", 2, 517, 3, 12, rhs="zero", tol=1.0, max_iter=10, shifts=SH_SLOW, d="wide",
        note="the mean over a 0 / 0 column is NaN and never stops the loop: max_iter + 2 iterations, not converged")
    # ---- operands: one case per rule for the number of q . K q partials
    add("operand-dense-mfma", "operands", "dense", 2, 517, 3, 3, note="9 partials per member (64-row tiles), S = 2")
    add("operand-dense-valu16", "operands", "dense", 2, 517, 1, 3, note="33 partials per member (16-row workgroups)")
    add("operand-dense-small", "operands", "dense", 2, 100, 3, 3, note="N < 256: 7 partials, S = 1")
    add("operand-dense-valu32", "operands", "dense", 128, 260, 1, 3, note="1024 workgroups reached at 32 rows: 9 partials")
    add("operand-kron-3x5", "operands", "kron", 2, 15, 3, 3, kron=(3, 5), note="unfused: vec_dot_part")
    add("operand-kron-128x128", "operands", "kron", 1, 16384, 1, 3, kron=(128, 128),
        note="fused: 1 partial per member against S = 64")
    add("operand-toeplitz", "operands", "toeplitz", 2, 517, 3, 3, note="the shared vec_dot_part epilogue")
    add("operand-sum", "operands", "sum", 2, 517, 3, 3, note="sum_descriptor(low-rank, dense) + diagonal")
    add("operand-closure", "operands", "closure", 2, 517, 3, 3, note="an opaque callback")
    add("operand-closure-c1", "operands", "closure", 2, 517, 1, 3)
    add("operand-tensor", "operands", "tensor", 2, 517, 3, 3, note="a dense tensor handed to utils.minres as the closure")
    # ---- preconditioners: the systems are K + sigma P
    pre_sh = (0.4, 1.1)
    add("precond-woodbury-r1-N517", "preconditioners", "lowrank", 2, 517, 3, 3, shifts=pre_sh, precond=("woodbury", 1))
    add("precond-woodbury-r5-N1030", "preconditioners", "lowrank", 2, 1030, 3, 3, shifts=pre_sh, precond=("woodbury", 5))
    add("precond-woodbury-r8-N517", "preconditioners", "lowrank", 2, 517, 3, 3, shifts=pre_sh, precond=("woodbury", 8))
    add("precond-woodbury-r8-N1030", "preconditioners", "lowrank", 2, 1030, 1, 3, shifts=pre_sh, precond=("woodbury", 8))
    add("precond-diag-N517", "preconditioners", "lowrank", 2, 517, 3, 3, shifts=pre_sh, precond="diag")
    add("precond-diag-N1030", "preconditioners", "closure", 2, 1030, 3, 3, shifts=pre_sh, precond="diag")
    # ---- stopping (tolerance > 0; the tolerances sit 4 x away from the float64 conv at every check: asserted on the CPU)
    add("stop-at-10", "stopping", "lowrank", 2, 517, 3, 10, tol=0.2, max_iter=30, shifts=SH_SLOW, d="wide")
    add("stop-at-20", "stopping", "lowrank", 2, 517, 3, 20, tol=7.5e-3, max_iter=40, shifts=(0.0, 0.002), d="wide", dlo=0.035,
        seed=8606, note="d in [0.035, 1.5]: conv falls 26 x between the two checks and the iterate still moves at step 21")
    add("stop-runs-out", "stopping", "lowrank", 2, 517, 3, 10, tol=1e-3, max_iter=8, shifts=SH_SLOW, d="wide",
        note="the check fires on the last iteration and does not pass")
    add("stop-max-iter-0", "stopping", "lowrank", 2, 517, 3, 2, tol=1e-4, max_iter=0)
    # ---- the wrapper utils.minres
    add("wrapper-cap-N6", "wrapper", "lowrank", 2, 6, 3, 9, tol=1e-4, max_iter=1000, wrapper="cap", still_moving=False,
        note="max_iter is capped at N + 1: nine iterations, the last three beyond the Krylov space (beta clamped at eps)")
    add("wrapper-broadcast", "wrapper", "lowrank", 2, 517, 3, 3, wrapper="broadcast",
        note="a [N, c] right-hand side against a B = 2 operator")
    # ---- float64 engine
    def add64(name, kind, B, N, c, k, **kw):
        add("f64-" + name, "float64", kind, B, N, c, k, dtype="f64", **kw)

    add64("dense-B1-N3-c1", "f64dense", 1, 3, 1, 3)
    add64("dense-B3-N64-c3", "f64dense", 3, 64, 3, 3, shifts=(0.0, 0.7, 2.0))
    add64("dense-B1-N257-c7", "f64dense", 1, 257, 7, 5)
    add64("dense-B3-N517-c3-member", "f64dense", 3, 517, 3, 3, shifts=0.1 * (1 + np.arange(6.0)).reshape(2, 3),
          per_member=True)
    add64("dense-value-1", "f64dense", 3, 64, 3, 3, shifts=lambda lam: np.ceil(lam) + np.array([1.0, 10.0]), value=-1.0)
    add64("dense-zero-column", "f64dense", 3, 64, 3, 3, rhs="zero")
    add64("dense-stop-at-10", "f64dense", 1, 257, 7, 10, tol=0.2, max_iter=30, shifts=SH_SLOW, d="wide")
    add64("closure", "f64closure", 3, 64, 3, 3)
    add64("lowrank-desc", "f64lowrank", 3, 517, 3, 3)
    add64("kron-desc", "f64kron", 2, 15, 3, 3, kron=(3, 5))
    add64("precond-pair", "f64dense", 3, 257, 3, 3, shifts=pre_sh, precond=("woodbury", 5))
    add64("precond-closure", "f64dense", 3, 257, 3, 3, shifts=pre_sh, precond="diag")
    add64("grid-refused", "f64dense", 1, 3, 1, 3, shifts=np.zeros(65536), refused="grid",
          note="Q B > 65535: refused before any launch")
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
RUNNABLE = tuple(c.name for c in CASES if "refused" not in c.opts)
REFUSED = tuple(c.name for c in CASES if "refused" in c.opts)
F32_CASES = tuple(n for n in RUNNABLE if BY_NAME[n].dtype == "f32")
F64_CASES = tuple(n for n in RUNNABLE if BY_NAME[n].dtype == "f64")
STOPPING = tuple(n for n in RUNNABLE if BY_NAME[n].tol > 0 and BY_NAME[n].k >= 10)


# ---- operands ------------------------------------------------------------------------------------------------------------
def _toeplitz_dense(col):
    n = col.shape[-1]
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return col[..., idx]


def _sym(K64, dt):
    return ((K64 + np.swapaxes(K64, -1, -2)) * 0.5).astype(dt)  # (symmetric bit for bit)


@functools.lru_cache(maxsize=None)
def operands(name):
    """The seeded operands of a case in the precision the device gets them (built in float64, rounded once): rhs [B,N,c],
    shifts [Q] | [Q,B], d [B,N], and by kind C [B,N,R] / K [B,N,N] / K1, K2 / col [B,N]; L [B,N,rank] of a Woodbury
    preconditioner, p [B,N] of the diagonal one."""
    c = BY_NAME[name]
    dt = f32 if c.dtype == "f32" else f64
    g = np.random.default_rng(c.seed)
    B, N = c.B, c.N
    o = {}
    dspec = c.opts.get("d", "unit")
    if dspec == "clusters":
        d = np.where(g.random((B, N)) < 0.5, 0.5, 1.5) + 0.2 * g.random((B, N))
    else:
        lo = c.opts.get("dlo", 0.02) if dspec == "wide" else 0.5
        d = lo + (1.5 - lo) * g.random((B, N))
    o["d"] = d.astype(dt)
    r = min(R, N)
    cscale = c.opts.get("cscale", 0.03 if dspec == "wide" else 1.0)
    C = (cscale * g.standard_normal((B, N, r)) / np.sqrt(r)).astype(dt)
    if c.kind in ("lowrank", "closure", "sum", "f64lowrank"):
        o["C"] = C
    if c.kind in ("dense", "tensor", "sum", "f64dense", "f64closure"):
        X = C.astype(f64) if c.kind != "sum" else g.standard_normal((B, N, 4)) / 2.0
        o["K"] = _sym(X @ np.swapaxes(X, -1, -2), dt)
    if c.kind in ("kron", "f64kron"):
        n1, n2 = c.opts["kron"]
        X1, X2 = g.standard_normal((B, n1, n1)) / np.sqrt(n1), g.standard_normal((B, n2, n2)) / np.sqrt(n2)
        o["K1"] = _sym(X1 @ np.swapaxes(X1, -1, -2) + 0.1 * np.eye(n1), dt)
        o["K2"] = _sym(X2 @ np.swapaxes(X2, -1, -2) + 0.1 * np.eye(n2), dt)
    if c.kind == "toeplitz":
        ell = 3.0 + 2.0 * g.random((B, 1))
        o["col"] = np.exp(-0.5 * (np.arange(N)[None, :] / ell) ** 2).astype(dt)
    rhs = g.standard_normal((B, N, c.c))
    if c.opts.get("rhs") == "scales":
        rhs = rhs * np.array([1.0, 1e3, 1e-3])
    if c.opts.get("rhs") == "zero":
        rhs[-1, :, -1] = 0.0
    if c.opts.get("wrapper") == "broadcast":  # (the device gets rhs[0] alone)
        rhs[1:] = rhs[:1]
    o["rhs"] = rhs.astype(dt)
    if isinstance(c.precond, tuple):
        k = c.precond[1]
        o["L"] = (0.5 * g.standard_normal((B, N, k)) / np.sqrt(k)).astype(dt)
        o["pd"] = (0.5 + g.random((B, N))).astype(dt)
    elif c.precond == "diag":
        o["p"] = (0.5 + g.random((B, N))).astype(dt)
    sh = c.opts["shifts"]
    if callable(sh):
        sh = sh(float(lam_max(_matmul(c, o, f64), B, N)))
    o["shifts"] = np.asarray(sh, dtype=dt)
    assert o["shifts"].shape == ((c.Q, B) if c.per_member else (c.Q,)), (name, o["shifts"].shape)
    return o


def lam_max(mm, B, N, iters=300):
    """Largest eigenvalue over the members of a positive definite operator, by power iteration (rounded up by its user)."""
    x = np.ones((B, N, 1))
    for _ in range(iters):
        x = mm(x)
        lam = np.sqrt((x * x).sum(-2, keepdims=True))
        x = x / lam
    return lam.max()


def _matmul(c, o, dt):
    """v -> K v (without `value`) in `dt`, the operands cast to it."""
    a = {k: v.astype(dt) for k, v in o.items() if k in ("C", "K", "K1", "K2", "d")}
    if "col" in o:
        a["K"] = _toeplitz_dense(o["col"].astype(dt))
    if c.kind in ("lowrank", "closure", "f64lowrank"):
        return lambda v: orc.matvec_lowrank_diag(a["C"], a["d"], v)
    if c.kind in ("kron", "f64kron"):
        return lambda v: orc.matvec_kron_diag(a["K1"], a["K2"], a["d"], v)
    if c.kind == "sum":
        return lambda v: orc.matvec_lowrank_diag(a["C"], None, v) + orc.matvec_dense_diag(a["K"], a["d"], v)
    return lambda v: orc.matvec_dense_diag(a["K"], a["d"], v)


def matmul(name, dt):
    return _matmul(BY_NAME[name], operands(name), dt)


def dense_tensor(name):
    """K + diag(d) of a "tensor" case written out in the device precision (one rounding more than the descriptor's
    operands: the references of such a case multiply by THIS matrix)."""
    o = operands(name)
    return (o["K"].astype(f64) + np.stack([np.diag(x) for x in o["d"].astype(f64)])).astype(o["K"].dtype)


def _tensor_matmul(name, dt):
    A = dense_tensor(name).astype(dt)
    return lambda v: np.matmul(A, v)


def operator(name, dt):
    return _tensor_matmul(name, dt) if BY_NAME[name].kind == "tensor" else matmul(name, dt)


@functools.lru_cache(maxsize=None)
def _precond64(name):
    """(P^-1 [B,N,N], P [B,N,N]) in float64, formed from the case's L, d (Woodbury) or p (diagonal); None without one."""
    c, o = BY_NAME[name], operands(name)
    if c.precond is None:
        return None
    if c.precond == "diag":
        p = o["p"].astype(f64)
        return np.stack([np.diag(1.0 / x) for x in p]), np.stack([np.diag(x) for x in p])
    L = o["L"].astype(f64)
    P = L @ np.swapaxes(L, -1, -2) + np.stack([np.diag(x) for x in o["pd"].astype(f64)])
    return np.linalg.inv(P), P


def preconditioner(name, dt):
    """v -> P^-1 v for the oracle: in float64 the inverse written out, in float32 what a float32 implementation applies
    (the QR form of oracle.lo_oracle.Preconditioner, the division by p)."""
    c, o = BY_NAME[name], operands(name)
    if c.precond is None:
        return None
    if dt == f64:
        Pinv = _precond64(name)[0]
        return lambda v: np.matmul(Pinv, v)
    if c.precond == "diag":
        return lambda v: v / o["p"][..., None]
    return orc.Preconditioner(o["L"], o["pd"]).apply


def woodbury_pair64(name):
    """(Q, noise) of the float64 engine's native preconditioner pair: P^-1 r = r / noise - Q (Q^T r)."""
    o = operands(name)
    pre = orc.Preconditioner(o["L"].astype(f64), o["pd"].astype(f64))
    return pre.Q, o["pd"].astype(f64)


# ---- references ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _steps(name, prec, k):
    """x [Q,B,N,c] after exactly k iterations (tolerance 0) of the oracle in float32 ("f32") or float64 ("f64")."""
    c, o = BY_NAME[name], operands(name)
    dt = f32 if prec == "f32" else f64
    with np.errstate(all="ignore"):
        x, info = orc.minres(operator(name, dt), o["rhs"].astype(dt), shifts=o["shifts"].astype(dt), value=c.value,
                             max_iter=k - 2, preconditioner=preconditioner(name, dt), tolerance=0.0)
    assert info.iterations == min(k, c.N + 3), (name, k, info.iterations)
    x = x.reshape((c.Q, c.B, c.N, c.c))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _run(name, prec):
    """(x [Q,B,N,c], info) of the oracle's run with the case's own tolerance and max_iter."""
    c, o = BY_NAME[name], operands(name)
    dt = f32 if prec == "f32" else f64
    with np.errstate(all="ignore"):
        x, info = orc.minres(operator(name, dt), o["rhs"].astype(dt), shifts=o["shifts"].astype(dt), value=c.value,
                             max_iter=c.max_iter, preconditioner=preconditioner(name, dt), tolerance=c.tol)
    x = x.reshape((c.Q, c.B, c.N, c.c))
    x.setflags(write=False)
    return x, info


def _conv(name, prec, k):
    """mean over (shift, member, column) of ||x_k - x_(k-1)|| / ||x_k||: what the stop test evaluates at iteration k."""
    a, b = (_steps(name, prec, j).astype(f64) for j in (k, k - 1))
    with np.errstate(all="ignore"):
        return float((np.sqrt(((a - b) ** 2).sum(-2)) / np.sqrt((a * a).sum(-2))).mean())


@functools.lru_cache(maxsize=None)
def reference(name, prec="f64"):
    """(x_k, info, {10: conv, 20: conv, ..}) of the oracle's run; conv at every check the run makes."""
    c = BY_NAME[name]
    x, info = _run(name, prec)
    return x, info, {j: _conv(name, prec, j) for j in range(10, info.iterations + 1, 10)}


def oracle_f32(name):
    return reference(name, "f32")


def _shifts_qb(name):
    c, o = BY_NAME[name], operands(name)
    sh = o["shifts"].astype(f64)
    return sh if c.per_member else np.repeat(sh[:, None], c.B, axis=1)


def system64(name):
    """x [B,N,c], sigma [B] -> (value K + sigma I) x, or (value K + sigma P) x, in float64."""
    c = BY_NAME[name]
    mm = operator(name, f64)
    val = 1.0 if c.value is None else c.value
    pre = _precond64(name)

    def apply(x, sigma):
        px = x if pre is None else np.matmul(pre[1], x)
        return val * mm(x) + sigma[:, None, None] * px

    return apply


@functools.lru_cache(maxsize=None)
def krylov(name):
    """The Krylov minimiser x_k [Q,B,N,c] of an unpreconditioned case with k <= KRYLOV_MAX_K, in float64."""
    c, o = BY_NAME[name], operands(name)
    assert c.precond is None and c.k <= KRYLOV_MAX_K and c.tol == 0.0, name
    M, sh = system64(name), _shifts_qb(name)
    b = o["rhs"].astype(f64)
    nb = np.sqrt((b * b).sum(-2, keepdims=True))
    zero = nb < 1e-10
    k = min(c.k, c.N)
    out = np.zeros((c.Q, c.B, c.N, c.c))
    for q in range(c.Q):
        V = [np.where(zero, 0.0, b / np.where(zero, 1.0, nb))]
        for _ in range(k - 1):
            w = M(V[-1], sh[q])
            for _ in range(2):
                for v in V:
                    w = w - v * (v * w).sum(-2, keepdims=True)
            V.append(w / np.where(zero, 1.0, np.sqrt((w * w).sum(-2, keepdims=True))))
        A = np.stack([M(v, sh[q]) for v in V], axis=-1)           # [B, N, c, k]
        A = np.moveaxis(A, 1, 2)                                   # [B, c, N, k]
        Qm, Rm = np.linalg.qr(A)
        rhs = np.swapaxes(Qm, -1, -2) @ np.moveaxis(b, 1, 2)[..., None]
        keep = ~zero[:, 0, :]
        y = np.zeros(rhs.shape)
        y[keep] = np.linalg.solve(Rm[keep], rhs[keep])
        x = (np.stack(V, axis=-1) * y[..., 0][:, None, :, :]).sum(-1)
        out[q] = np.where(zero, 0.0, x)
    return out


# ---- the checker ---------------------------------------------------------------------------------------------------------
def rel_err(x, ref):
    """||x - ref|| / ||ref|| over N, per (shift, member, column); 0 where ref is all zero."""
    x, ref = np.asarray(x, f64), np.asarray(ref, f64)
    den = np.sqrt((ref * ref).sum(-2))
    with np.errstate(all="ignore"):
        return np.where(den == 0, 0.0, np.sqrt(((x - ref) ** 2).sum(-2)) / np.where(den == 0, 1.0, den))


def residuals(name, x):
    """||b - M x|| / ||b|| per (shift, member, column); 0 for a zero right-hand-side column."""
    c, o = BY_NAME[name], operands(name)
    M, sh = system64(name), _shifts_qb(name)
    b = o["rhs"].astype(f64)
    nb = np.sqrt((b * b).sum(-2))
    x = np.asarray(x, f64)
    out = np.zeros((c.Q, c.B, c.c))
    for q in range(c.Q):
        r = b - M(x[q], sh[q])
        out[q] = np.where(nb < 1e-10, 0.0, np.sqrt((r * r).sum(-2)) / np.where(nb < 1e-10, 1.0, nb))
    return out


@functools.lru_cache(maxsize=None)
def _reference_residuals(name):
    return residuals(name, reference(name)[0])


def check(name, x):
    """The figures of the module docstring for an output x [Q,B,N,c]: dict(err, resid: the worst values; err_all,
    resid_all [Q,B,c]; zeros: non-zero (or non-finite) entries in the columns whose right-hand side is zero)."""
    c, o = BY_NAME[name], operands(name)
    x = np.asarray(x)
    assert x.shape == (c.Q, c.B, c.N, c.c), (name, x.shape)
    zero = np.sqrt((o["rhs"].astype(f64) ** 2).sum(-2)) < 1e-10          # [B, c]
    x64 = x.astype(f64)
    zeros = int(((x64 != 0) & zero[None, :, None, :]).sum())
    x64 = np.where(zero[None, :, None, :], 0.0, x64)
    err = rel_err(x64, reference(name)[0])
    err = np.where(np.isfinite(err), err, np.inf)
    res = np.abs(residuals(name, x64) - _reference_residuals(name))
    res = np.where(np.isfinite(res), res, np.inf)
    return dict(err=float(err.max()), resid=float(res.max()), err_all=err, resid_all=res, zeros=zeros)


@functools.lru_cache(maxsize=None)
def oracle_values(name):
    """check() of the float32 oracle's run (float32 cases)."""
    return check(name, oracle_f32(name)[0])


def bounds(name):
    """{err, resid} -> bound.  float32: clamp(FACTOR x the float32 oracle's figure, FLOOR, CAP); float64: F64_BOUND."""
    if BY_NAME[name].dtype == "f64":
        return dict(err=F64_BOUND, resid=F64_BOUND)
    v = oracle_values(name)
    return {k: float(min(max(FACTOR * v[k], FLOOR), CAP)) for k in ("err", "resid")}


def violations(vals, bnd):
    bad = [k for k in ("err", "resid") if not vals[k] <= bnd[k]]
    return bad + (["zeros"] if vals["zeros"] else [])


def conv_bound(name, at):
    """Relative bound on info.conv of a run whose last check was at iteration `at`."""
    ref = reference(name)[2][at]
    if BY_NAME[name].dtype == "f64":
        return CONV_FLOOR
    return max(FACTOR * abs(oracle_f32(name)[2][at] - ref) / ref, CONV_FLOOR)


def movement(name):
    """min over (shift, member, column) of ||x_k - x_j|| / ||x_k|| in the float64 oracle, for j = k - 1 and -- while
    the Krylov space is not exhausted (k < N) -- j = k + 1: how far an off-by-one step count or a stale search vector
    would move the result.  The k-th iterate is the run's own result (for a stopping case: where it stopped)."""
    c = BY_NAME[name]
    xk = reference(name)[0].astype(f64)
    k = reference(name)[1].iterations
    zero = np.sqrt((xk * xk).sum(-2)) == 0
    worst = np.inf
    for j in (k - 1, k + 1):
        if j < 1 or (j > k and k >= c.N):
            continue
        e = rel_err(_steps(name, "f64", j), xk)
        worst = min(worst, float(np.where(zero, np.inf, e).min()))
    return worst


def tag(name, vals, bnd):
    """One line: the case, S, and per figure the value / the float32 oracle's / the bound (float64: the value / the bound),
    then the worst value over its bound."""
    c = BY_NAME[name]
    worst = max(vals[k] / bnd[k] for k in ("err", "resid"))
    if c.dtype == "f64":
        return f"{name:28s} " + "  ".join(f"{k} {vals[k]:.1e}/{bnd[k]:.0e}" for k in ("err", "resid")) + f"  worst {worst:.0e}"
    ref, S = oracle_values(name), choose_split(c.B, c.N)[0]
    return (f"{name:28s} S={S:<3d} " + "  ".join(f"{k} {vals[k]:.1e}/{ref[k]:.1e}/{bnd[k]:.1e}" for k in ("err", "resid"))
            + f"  worst {worst:.3f}")
