"""Every step route of the Lanczos tridiagonalisation (csrc/lo_lanczos.hip, csrc/lo_lanczos_f64.hip) as a table of tiny
cases, shared by tests/test_lanczos_invariants_cpu.py (the oracle against the checker, the checker's teeth, the stop
conditions the table relies on; no GPU) and tests/test_gpu_lanczos_routes.py (the kernels).  Everything here is numpy:
the case table with the route the host code must take, the seeded operands, the oracle's runs of them, the checker and
the bounds.  Not a test module.

A trajectory comparison cannot pin a float32 Lanczos run: it leaves any reference run after a few steps.  The
decomposition itself is unique, though (implicit-Q theorem): q_0 = v / ||v||, Q^T Q = I, Q^T A Q = T tridiagonal with
positive symmetric off-diagonals together fix every entry the kernels write, and all of it can be evaluated in float64
(in long double for a float64 run) from the returned Q and T and the exact A, whatever rounding path the run took.
`check_lanczos` returns

    q0     max |q[..., 0] - v / ||v|||
    orth   max |Q^T Q - I|
    proj   max |Q^T A Q - T| / ||A||_2   over the WHOLE k x k matrix: every alpha and beta, the zeros off the tridiagonal
    resid  max |(A Q - Q T)[:, :k-1]| / ||A||_2
    recon  max |Q T Q^T - A| / ||A||_2   only when k == N
    sym    max |T - T^T|                 must be exactly 0
    offmin min of the off-diagonals      must be >= 0

Bounds (`bounds`): for q0 / orth / proj / resid / recon 8 x the value the ORACLE's run in the same precision gives on
the same inputs (the kernels sum in slices and trees instead of numpy's order, and the fused route's alpha carries one
more product term), never more than 1e-4 in float32 (the orthogonality bar of tests/test_gpu_sweep.py) and 1e-10 in
float64.  The bounds come from the oracle, never from the library."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cases  # noqa: E402  (tests/golden/cases.py: the seeded operand recipes)
from oracle import lo_oracle as orc  # noqa: E402  (the checker)

f32, f64 = np.float32, np.float64
FACTOR = 8.0
CAP = {"f32": 1e-4, "f64": 1e-10}
BOUNDED = ("q0", "orth", "proj", "resid", "recon")

# constants of csrc/lo_lanczos.hip the table is built around
FUSED_Q = 20      # kLzFusedQ: the fused step takes min(max_iter, N) <= FUSED_Q + 1
MAX_Q = 24        # kLzMaxQ: more stored vectors run k_lz_multidot_any / k_lz_correct_any
VEC4_P = (4, 8, 16, 32, 64)


class Case:
    """One call of lanczos_tridiag.  kind: "lowrank" (C C^T + diag d, a descriptor), "dense" (the same matrix written
    out, a dense descriptor), "closure" (the same operator as a callback), "rank1" (u u^T, ||u|| = 1, no diagonal: a
    low-rank descriptor with R = 1 and no diagonal), "mixed" (member 0 the rank-one operator, member 1 low-rank +
    diagonal).  route: what the host code must run --
      fused   k_lz_alpha, k_lz_dots_fused, k_lz_reduce_pred, k_lz_correct_check, k_lz_finish
      alpha   the fused loop's alpha-only branch and nothing else (two steps)
      plain4  k_lz_sub_prev_dot with the float4 multidot / correct kernels
      scalar  k_lz_sub_prev_dot with the scalar kernels
      none    a single step: no loop at all
    unfused: run under LO_LZ_UNFUSED.  steps: vectors the run must return (None: min(max_iter, N); -1: not pinned).
    members: the batch members the invariants are asserted on (None: all)."""

    def __init__(self, name, B, N, R, P, max_iter, route, kind="lowrank", unfused=False, steps=None, members=None,
                 seed=0, note=""):
        self.name, self.B, self.N, self.R, self.P, self.max_iter = name, B, N, R, P, max_iter
        self.route, self.kind, self.unfused, self.members = route, kind, unfused, members
        self.seed, self.note = seed, note
        self.num_iter = min(max_iter, N)
        self.steps = self.num_iter if steps is None else steps

    def __repr__(self):
        return self.name


def expected_route(c):
    """The selection of lo_lanczos_tridiag_f32 restated (every operand of the table writes <= 64 dot partials)."""
    if c.num_iter == 1:
        return "none"
    if c.P in VEC4_P and c.num_iter <= FUSED_Q + 1 and not c.unfused:
        return "alpha" if c.num_iter == 2 else "fused"
    return "plain4" if c.P in VEC4_P else "scalar"


def _table():
    t = []

    def add(*a, **kw):
        t.append(Case(*a, seed=7000 + 10 * len(t), **kw))

    # ---- fused route
    add("fused-N517-P4-k21", 2, 517, 8, 4, 21, "fused",
        note="two row slices, the second of 257 rows; nq reaches 20 = MAXQ; the last step takes the alpha-only branch")
    for P in (8, 32, 64):
        add(f"fused-N260-P{P}-k20", 1, 260, 5, P, 20, "fused",
            note="P = 64: c2 = 32 in k_lz_correct_check, 21 x 64 items in k_lz_reduce_pred")
    add("fused-N1030-P16-k7", 3, 1030, 8, 16, 7, "fused", note="four slices, the last of 250 rows")
    add("fused-N6-P4-k9", 1, 6, 3, 4, 9, "fused", note="num_iter = N = 6, one short slice; Q T Q^T = A")
    add("fused-N260-P4-k2", 1, 260, 5, 4, 2, "alpha", note="the loop runs only its alpha branch")
    # (both run fused: the dense matvec writes one dot partial per 16-row workgroup, 33 <= 64 slots; a closure's
    #  partials come from vec_dot_part over the 2 row slices, not from a matvec epilogue)
    add("dense-N517-P4-k12", 2, 517, 8, 4, 12, "fused", kind="dense",
        note="dot partials of the dense matvec's own workgroups")
    add("closure-N517-P4-k12", 2, 517, 8, 4, 12, "fused", kind="closure",
        note="dot partials from vec_dot_part, not an epilogue")
    # ---- plain route, float4
    add("plain4-N517-P4-k22", 2, 517, 8, 4, 22, "plain4", note="one past the fused limit")
    add("plain4-N300-P8-k26", 1, 300, 8, 8, 26, "plain4",
        note="nq goes 24 -> 25: the <24> kernels, then the _any pair, in one run")
    add("plain4-N40-P4-k40", 2, 40, 4, 4, 40, "plain4", note="num_iter = N = 40; Q T Q^T = A")
    add("unfused-N517-P4-k21", 2, 517, 8, 4, 21, "plain4", unfused=True,
        note="the first fused case under LO_LZ_UNFUSED")
    add("unfused-N260-P64-k20", 1, 260, 5, 64, 20, "plain4", unfused=True,
        note="the P = 64 fused case under LO_LZ_UNFUSED")
    # ---- plain route, scalar
    for P in (1, 2, 3, 5, 17):
        add(f"scalar-N517-P{P}-k12", 2, 517, 8, P, 12, "scalar", note="256 / P inexact: idle threads")
    for P in (100, 128, 200, 256):
        add(f"scalar-N64-P{P}-k6", 1, 64, 5, P, 6, "scalar",
            note="2 or 1 rows per pass; 56 idle threads at P = 200; kMaxCols at P = 256; a power of two outside the float4 set")
    add("scalar-N64-P3-k30", 1, 64, 5, 3, 30, "scalar", note="nq > 24 on the scalar route")
    add("scalar-N3-P1-k5", 1, 3, 2, 1, 5, "scalar", note="num_iter = 3")
    for P in (3, 4):
        add(f"single-N517-P{P}-k1", 2, 517, 8, P, 1, "none", note="T = [[q0^T A q0]], Q = q0")
    # ---- early stop: the Krylov space of u u^T has dimension 2
    add("stop-fused-P4", 1, 300, 1, 4, 10, "fused", kind="rank1", steps=2)
    add("stop-plain4-P4", 1, 300, 1, 4, 10, "plain4", kind="rank1", steps=2, unfused=True)
    add("stop-scalar-P3", 1, 300, 1, 3, 10, "scalar", kind="rank1", steps=2)
    # ---- batch-global stop: member 0 exhausted after two vectors, member 1 not
    add("global-stop-P4", 2, 300, 8, 4, 10, "fused", kind="mixed", steps=-1, members=(1,),
        note="a per-member stop flag, or one keeping the last writer's value, would return 2 vectors")
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
STOP_CASES = tuple(c for c in CASES if c.kind == "rank1")
GLOBAL_STOP = BY_NAME["global-stop-P4"]

# float64 entry (csrc/lo_lanczos_f64.hip): (P, N, max_iter), B = 2
F64_SHAPES = tuple((P, N, k) for P in (1, 3, 4) for N in (37, 517) for k in (1, 2, 12)) + tuple((P, 6, 9) for P in (1, 3, 4))
F64_B, F64_R = 2, 8
F64_DESC_SHAPE = (3, 517, 12)
F64_STOP = (4, 300, 10)  # (P, N, max_iter) of the rank-one early stop, B = 1


def _unit(seed, N, dtype):
    u = cases.randn(seed, 1, N, 1, dtype=dtype)
    return (u / np.sqrt((u.astype(f64) ** 2).sum())).astype(dtype)


@functools.lru_cache(maxsize=None)
def operands(name):
    """float32 operands of a case and the exact matrix they stand for: dict(C [B,N,R], d [B,N] or None, V [B,N,P],
    K [B,N,N] float32 (kind "dense" only), A64 [B,N,N] formed from the float32 operands cast to float64, normA [B])."""
    c = BY_NAME[name]
    C, d, _ = cases.lowrank_diag(c.seed, c.B, c.N, c.R, 1)
    V = cases.randn(c.seed + 1, c.B, c.N, c.P, dtype=f32)
    out = {}
    if c.kind == "rank1":
        C, d = _unit(c.seed + 2, c.N, f32), None
    elif c.kind == "mixed":
        C[0], d[0] = 0.0, 0.0
        C[0, :, :1] = _unit(c.seed + 2, c.N, f32)[0]
    if c.kind == "dense":
        C64 = C.astype(f64)
        K64 = C64 @ np.swapaxes(C64, -1, -2)
        out["K"] = ((K64 + np.swapaxes(K64, -1, -2)) * 0.5).astype(f32)  # (symmetric bit for bit)
        A64 = out["K"].astype(f64)
    else:
        C64 = C.astype(f64)
        A64 = C64 @ np.swapaxes(C64, -1, -2)
    if d is not None:
        A64 = A64 + np.stack([np.diag(x) for x in d.astype(f64)])
    out.update(C=C, d=d, V=V, A64=A64, normA=np.abs(np.linalg.eigvalsh(A64)).max(-1))
    return out


def matmul_closure(name, dtype):
    """The operator of a case as the oracle's closure, in `dtype`."""
    o = operands(name)
    if "K" in o:
        K, d = o["K"].astype(dtype), o["d"].astype(dtype)
        return lambda x: orc.matvec_dense_diag(K, d, x)
    C, d = o["C"].astype(dtype), None if o["d"] is None else o["d"].astype(dtype)
    return lambda x: orc.matvec_lowrank_diag(C, d, x)


@functools.lru_cache(maxsize=None)
def oracle_run(name, prec):
    """(q, t) of oracle.lo_oracle.lanczos_tridiag on the case's operands in float32 ("f32") or float64 ("f64")."""
    c = BY_NAME[name]
    dt = f32 if prec == "f32" else f64
    with np.errstate(all="ignore"):  # (an exhausted member divides noise by noise)
        return orc.lanczos_tridiag(matmul_closure(name, dt), c.max_iter, operands(name)["V"].astype(dt))


def _members(c, q, t, A64, normA, V):
    """Restrict everything to the members the case asserts on; q, t with their probe dimension."""
    if q.ndim == V.ndim:
        q, t = q[None], t[None]
    if c is None or c.members is None:
        return q, t, A64, normA, V
    m = list(c.members)
    return q[:, m], t[:, m], A64[m], normA[m], V[m]


def check_lanczos(q, t, A64, init64, normA=None, wide=False):
    """The invariants of a Lanczos run, in float64.  q [P,*B,N,k], t [P,*B,k,k] (squeezed for P == 1, as the API returns
    them), A64 [*B,N,N] (or a callable X [P,*B,N,k] -> A X together with `normA`), init64 [*B,N,P].  Returns the dict of
    the module docstring (worst value over probes and members).  wide: evaluate in numpy's long double instead -- for
    float64 RUNS, whose own rounding a float64 evaluation would hide (the oracle's q0 against v / ||v|| in the same
    arithmetic is exactly 0, and 8 x 0 is no bound)."""
    dt = np.longdouble if wide else f64
    apply = A64 if callable(A64) else None
    q, t, init64 = (np.asarray(a, dtype=dt) for a in (q, t, init64))
    if q.ndim == init64.ndim:
        q, t = q[None], t[None]
    N, k = q.shape[-2:]
    assert t.shape == q.shape[:-2] + (k, k) and init64.shape == q.shape[1:-2] + (N, q.shape[0]), (q.shape, t.shape)
    if apply is None:
        A64 = np.asarray(A64, dtype=dt)
        assert A64.shape == q.shape[1:-2] + (N, N), (q.shape, A64.shape)
        if normA is None:
            normA = np.abs(np.linalg.eigvalsh(A64.astype(f64))).max(-1)
    nrm = np.asarray(normA, dt)[None, ..., None, None]
    v = np.moveaxis(init64, -1, 0)  # [P, *B, N]
    qT = np.swapaxes(q, -1, -2)
    AQ = A64[None] @ q if apply is None else apply(q)
    out = {
        "q0": float(np.abs(q[..., 0] - v / np.sqrt((v * v).sum(-1, keepdims=True))).max()),
        "orth": float(np.abs(qT @ q - np.eye(k, dtype=dt)).max()),
        "proj": float((np.abs(qT @ AQ - t) / nrm).max()),
        "resid": float((np.abs((AQ - q @ t)[..., : k - 1]) / nrm).max()) if k > 1 else 0.0,
        "sym": float(np.abs(t - np.swapaxes(t, -1, -2)).max()),
        "offmin": float(np.diagonal(t, 1, -2, -1).min()) if k > 1 else np.inf,
    }
    if k == N and apply is None:
        out["recon"] = float((np.abs(q @ t @ qT - A64[None]) / nrm).max())
    return out


def lowrank_apply64(C, d, iters=200):
    """(X [P,*B,N,k] -> A X, ||A||_2 [*B]) of A = C C^T + diag d in float64 without writing A out, for shapes where
    [B, N, N] would not be small.  The norm by power iteration from the vector of ones, good to a percent: it only scales
    the quantities, the same way for the oracle's run and the kernels'."""
    C64, d64 = np.asarray(C, f64), np.asarray(d, f64)

    def apply(X):
        return C64 @ (np.swapaxes(C64, -1, -2) @ X) + d64[..., None] * X

    x = np.ones(C64.shape[:-1] + (1,))
    for _ in range(iters):
        x = apply(x)
        lam = np.sqrt((x * x).sum(-2, keepdims=True))
        x = x / lam
    return apply, lam[..., 0, 0]


def check_case(name, q, t, wide=False):
    """check_lanczos of a float32 case's result on the members the case asserts on."""
    c, o = BY_NAME[name], operands(name)
    q, t, A64, normA, V = _members(c, np.asarray(q), np.asarray(t), o["A64"], o["normA"], o["V"])
    return check_lanczos(q, t, A64, V.astype(f64), normA, wide=wide)


@functools.lru_cache(maxsize=None)
def oracle_values(name, prec):
    return check_case(name, *oracle_run(name, prec), wide=prec == "f64")


def bounds_from(oracle_vals, prec):
    return {k: min(FACTOR * v, CAP[prec]) for k, v in oracle_vals.items() if k in BOUNDED}


def bounds(name, prec="f32"):
    """The GPU bounds of a float32 case: FACTOR x the oracle's own value, capped."""
    return bounds_from(oracle_values(name, prec), prec)


def violations(vals, bnd):
    """Names of the quantities of `vals` that break `bnd`, the exact symmetry or the sign of the off-diagonals."""
    bad = [k for k in BOUNDED if k in vals and not vals[k] <= bnd[k]]
    if vals["sym"] != 0.0:
        bad.append("sym")
    if not vals["offmin"] >= 0.0:
        bad.append("offmin")
    return bad


def tag(name, vals, ref, bnd):
    """One line per quantity: the value, the oracle's, the bound."""
    rows = [f"{k}={vals[k]:.2e} (oracle {ref[k]:.2e}, bound {bnd[k]:.2e})" for k in BOUNDED if k in vals]
    return f"{name}: " + "; ".join(rows) + f"; sym={vals['sym']:.1e} offmin={vals['offmin']:.2e}"


# ---- float64 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f64_operands(P, N, max_iter, rank1=False):
    """float64 operands: C [B,N,R], d [B,N], the dense A = C C^T [B,N,N] (the diagonal apart), V [B,N,P], A64 = A + diag d.
    rank1: B = 1, A = u u^T, d = None."""
    seed = 7900 + 100 * P + N + max_iter
    if rank1:
        u = _unit(seed, N, f64)
        A = u @ np.swapaxes(u, -1, -2)
        return dict(C=u, d=None, A=A, V=cases.randn(seed + 1, 1, N, P, dtype=f64), A64=A)
    C, d, _ = cases.lowrank_diag(seed, F64_B, N, min(F64_R, N), 1, dtype=f64)
    A = C @ np.swapaxes(C, -1, -2)
    return dict(C=C, d=d, A=A, V=cases.randn(seed + 1, F64_B, N, P, dtype=f64),
                A64=A + np.stack([np.diag(x) for x in d]))


@functools.lru_cache(maxsize=None)
def f64_oracle(P, N, max_iter, rank1=False):
    """((q, t), check_lanczos values) of the oracle's float64 run on the dense matrix."""
    o = f64_operands(P, N, max_iter, rank1)
    with np.errstate(all="ignore"):
        q, t = orc.lanczos_tridiag(lambda x: orc.matvec_dense_diag(o["A"], o["d"], x), max_iter, o["V"])
    return (q, t), f64_check(P, N, max_iter, q, t, rank1)


def f64_check(P, N, max_iter, q, t, rank1=False):
    """check_lanczos of a float64 run, evaluated in long double on A + diag d formed in long double."""
    o = f64_operands(P, N, max_iter, rank1)
    A = o["A"].astype(np.longdouble)
    if o["d"] is not None:
        A = A + np.stack([np.diag(x) for x in o["d"]]).astype(np.longdouble)
    normA = np.abs(np.linalg.eigvalsh(o["A64"])).max(-1)
    return check_lanczos(q, t, A, o["V"], normA, wide=True)


# ---- root_from_lanczos -----------------------------------------------------------------------------------------------
U24 = 2.0 ** -24
# (P, B, N, k): one column; k = 16 = KM of <16>; 17 -> <32>; k = 32 = KM; P = 64 needs 125 KB of LDS in the native entry
ROOT_SHAPES = ((1, 2, 517, 1), (3, 2, 517, 16), (16, 2, 517, 17), (4, 1, 300, 32), (64, 1, 260, 20))
ROOT_NATIVE_UNSUPPORTED = ((64, 1, 260, 20),)
ROOT_TORCH_SHAPE = (2, 2, 100, 33)


@functools.lru_cache(maxsize=None)
def root_inputs(shape):
    """Synthetic inputs of the root epilogue: q [P,B,N,k] random, evecs [P,B,k,k] orthogonal up to float32 rounding,
    evals [P,B,k] uniform in [0.5, 2]; the three float64 references and |Q| |V|."""
    P, B, N, k = shape
    g = np.random.default_rng(7800 + P + 3 * N + 7 * k)
    q = g.standard_normal((P, B, N, k)).astype(f32)
    evecs = np.linalg.qr(g.standard_normal((P, B, k, k)))[0].astype(f32)
    evals = (0.5 + 1.5 * g.random((P, B, k))).astype(f32)
    qv = q.astype(f64) @ evecs.astype(f64)
    mag = np.abs(q).astype(f64) @ np.abs(evecs).astype(f64)
    s = np.sqrt(evals.astype(f64))[..., None, :]
    return dict(q=q, evecs=evecs, evals=evals, refs=(qv, qv * s, qv / s), mags=(mag, mag * s, mag / s))


def root_err_over_bound(shape, outs):
    """max over the three outputs and their elements of |out - ref| / ((k + 2) 2^-24 |Q| |V| scale): the float32
    dot-product bound (k products and sums, the square root, the scaling), derived, not measured."""
    r = root_inputs(shape)
    k = shape[-1]
    worst = 0.0
    for out, ref, mag in zip(outs, r["refs"], r["mags"]):
        out = np.asarray(out, dtype=f64)
        assert out.shape == ref.shape, (out.shape, ref.shape)
        worst = max(worst, float((np.abs(out - ref) / ((k + 2) * U24 * mag)).max()))
    return worst
