"""Edge cases of the backward contraction kernels (csrc/lo_bilinear.hip, `kron_bilinear` of csrc/lo_kron.hip) and of the
SLQ eigensolver (csrc/lo_eig.hip), shared by tests/test_bilinear_cases_cpu.py (the table's own preconditions and the
bounds, no GPU) and tests/test_gpu_backward_kernels.py (the kernels against the fp64 oracle).  Everything here is numpy:
the case tables, a restatement of every host-side selection rule as a route label, the seeded inputs, the fp64
references with their magnitudes, the rounding-chain counts K of the componentwise bound

    |got - ref64| <= gamma_K * mag,   gamma_K = K u / (1 - K u),  u = 2^-24,

a float32 emulation of every kernel's summation order, and the SLQ reference with its checks.  Not a test module.

`mag` is the reference formula on absolute values: every output is a sum of products of two or three inputs, each term
passes at most K roundings on its way to the output, so the error is at most gamma_K times the sum of the absolute
terms (Higham, Accuracy and Stability of Numerical Algorithms, 3.1-3.4: any summation order, the chain length is what
counts).  An addition to an exact zero (the first step of a chain, zero padding) rounds nothing."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lo_oracle as orc  # noqa: E402  (the checker)

f32, f64 = np.float32, np.float64
U24 = 2.0 ** -24
THREADS = 256   # kThreads
BD_TILE = 64    # kBdTile: output tile of k_bil_dense
BD_MAXD = 64    # kBdMaxD: columns per pass of k_bil_dense
BDIAG_LDS = 8192  # kBdiagLds: floats of LDS of k_bil_diag
GEMM_TILE = 64  # BM = BN of k_gemm
GEMM_BK = 16
EIG_MAX_T = 32  # kEigMaxT
LDS_BYTES = 64 * 1024


def cdiv(a, b):
    return -(-a // b)


def gamma(K):
    return K * U24 / (1.0 - K * U24)


def err_over_bound(got, ref, mag, K):
    """max over the components of |got - ref| / (gamma_K mag); a component whose magnitude is zero must be exact."""
    err = np.abs(np.asarray(got, f64) - ref)
    bound = gamma(K) * mag
    zero = bound == 0
    if (err[zero] != 0).any():
        return np.inf
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


def _rng(seed):
    return np.random.default_rng(seed)


def _normal(g, *shape):
    return g.standard_normal(shape).astype(f32)


# ---- dense: U V^T --------------------------------------------------------------------------------------------------
# (B, N, D), the label dense_route() must return
DENSE_CASES = (
    ((2, 1, 1), "passes1(dn1) grid1x1x2 edge1"),          # smallest shape
    ((2, 63, 64), "passes1(dn64) grid1x1x2 edge63"),      # one full pass
    ((2, 64, 65), "passes2(dn1) grid1x1x2 edge64"),       # exact tile; second pass with dn = 1
    ((2, 65, 130), "passes3(dn2) grid2x2x2 edge1"),       # 2 x 2 tiles, a one-row edge tile; passes 64 / 64 / 2
    ((1, 130, 3), "passes1(dn3) grid3x3x1 edge2"),        # 3 x 3 tiles
)


def dense_facts(B, N, D):
    """lo_bilinear_dense_f32: one launch per 64 columns of U / V (the first overwrites, the others accumulate), a grid
    of ceil(N / 64)^2 x B tiles."""
    passes = cdiv(D, BD_MAXD)
    tiles = cdiv(N, BD_TILE)
    return {"passes": passes, "dn_last": D - BD_MAXD * (passes - 1), "tiles": tiles, "edge": N - BD_TILE * (tiles - 1)}


def dense_route(B, N, D):
    f = dense_facts(B, N, D)
    return f"passes{f['passes']}(dn{f['dn_last']}) grid{f['tiles']}x{f['tiles']}x{B} edge{f['edge']}"


def dense_K(B, N, D):
    """A pass is a chain of dn <= 64 fmaf (one rounding each, the first onto 0.f); every later pass adds its
    accumulator to the output with one more rounding.  The first product of any pass is the longest chain:
    min(D, 64) + (passes - 1)."""
    return min(D, BD_MAXD) + dense_facts(B, N, D)["passes"] - 1


@functools.lru_cache(maxsize=None)
def dense_inputs(case):
    B, N, D = case
    g = _rng(4100 + 7 * N + D)
    U, V = _normal(g, B, N, D), _normal(g, B, N, D)
    ref = orc.bilinear_derivative_dense(U.astype(f64), V.astype(f64))
    mag = orc.bilinear_derivative_dense(np.abs(U).astype(f64), np.abs(V).astype(f64))
    return U, V, ref, mag


# ---- diag: sum_d U o V, and its sum over N ---------------------------------------------------------------------------
DIAG_CASES = (
    ((3, 100, 1), "rb256 blocks2 last44 spans"),      # a block spans members
    ((2, 257, 32), "rb256 blocks3 last2 spans"),      # rb = 256; tail block of 2 rows
    ((2, 130, 33), "rb248 blocks2 last12 spans"),     # rb = 248
    ((2, 7, 3000), "rb2 blocks7 last2 spans"),        # rb = 2
    ((1, 5, 8192), "rb1 blocks5 last1 nospan"),       # rb = 1; 8192 floats of LDS
    ((3, 1, 5), "rb256 blocks1 last3 spans"),         # N = 1
    ((2, 256, 2), "rb256 blocks2 last256 nospan"),    # k_bil_sum_rows: exactly one stride
)


def diag_facts(B, N, D):
    """lo_bilinear_diag_f32: workgroups of rb = min(256, 8192 / D) consecutive rows of the flattened [B N, D]."""
    rows = B * N
    rb = min(THREADS, BDIAG_LDS // D)
    blocks = cdiv(rows, rb)
    spans = any(k * rb // N != (min((k + 1) * rb, rows) - 1) // N for k in range(blocks))
    return {"rb": rb, "blocks": blocks, "last": rows - rb * (blocks - 1), "spans": spans, "strides": cdiv(N, THREADS)}


def diag_route(B, N, D):
    f = diag_facts(B, N, D)
    return f"rb{f['rb']} blocks{f['blocks']} last{f['last']} {'spans' if f['spans'] else 'nospan'}"


def diag_K(B, N, D, constant):
    """Full: every product is rounded (1), the row sum is a chain of D - 1 additions (the first lands on 0.f): D.
    Constant: k_bil_sum_rows adds ceil(N / 256) - 1 times per thread (again the first lands on 0.f), 6 butterfly steps
    of wave_sum, 2 levels of (r0 + r1) + (r2 + r3): D + ceil(N / 256) - 1 + 8."""
    return D + (cdiv(N, THREADS) - 1 + 8 if constant else 0)


@functools.lru_cache(maxsize=None)
def diag_inputs(case):
    B, N, D = case
    g = _rng(4200 + 7 * N + D)
    U, V = _normal(g, B, N, D), _normal(g, B, N, D)
    U64, V64 = U.astype(f64), V.astype(f64)
    out = {}
    for constant in (False, True):
        out[constant] = (orc.bilinear_derivative_diag(U64, V64, constant),
                         orc.bilinear_derivative_diag(np.abs(U64), np.abs(V64), constant))
    return U, V, out


# ---- root: U (V^T C) + V (U^T C) -------------------------------------------------------------------------------------
# (B, N, R, D)
ROOT_CASES = (
    ((2, 1, 1, 1), "S1x4 mfma1(1,nw4,tiles1)"),                          # smallest shape
    ((3, 33, 32, 32), "S1x36 mfma1(32,nw4,tiles1)"),                     # mfma1, full tile, odd N
    ((2, 300, 32, 33), "S1x300 mfma2(33,nw4,tiles1)"),                   # mfma2, one column in the second tile; DE = 34
    ((2, 257, 33, 62), "S1x260 valu(62,nw2,tiles1)"),                    # valu; 2046 pairs; RP = 64; nw = 2 at 64000 B
    ((2, 257, 48, 64), "S1x260 valu(42,nw4,tiles1) valu(22,nw4,tiles1)"),  # dmax = 42: chunks of 42 and 22
    ((1, 515, 5, 3), "S2x260 mfma1(3,nw4,tiles1)"),                      # S = 2; second slice of 255 rows
    ((2048, 129, 8, 4), "S1x132 mfma1(4,nw4,tiles8)"),                   # tiles = 8; grid x = 1; second tile has one row
)


def choose_split(B, N, min_rows, max_split=256):
    """csrc/lo_vec.hip:14-28: (S, rows per slice)."""
    S = cdiv(1024, B)
    maxS = max(1, N // max(min_rows, 4))
    S = max(1, min(S, maxS))
    cap = 64
    while cap < max_split and (cap * 2) * (cap * 2) * 16 <= N:
        cap *= 2
    S = min(S, min(cap, max_split))
    rows = cdiv(N, S)
    rows = cdiv(rows, 4) * 4
    return cdiv(N, rows), rows


def root_chunks(R, D):
    """kernels.bilinear_root: the column chunks [(d0, width)] of U / V one call of lo_bilinear_root_f32 takes."""
    rp = cdiv(R, 32) * 32
    dmax = max(1, min(2048 // R, (16000 // (2 * rp + 64)) & ~1))
    return [(d0, min(dmax, D - d0)) for d0 in range(0, D, dmax)]


def root_launch_facts(B, N, R, Dc):
    """lo_bilinear_root_f32 for one chunk of Dc columns: phase-A engine, the waves `nw` of a phase-B workgroup (as many
    32-row blocks as fit 64 KB of LDS), the row blocks `tiles` a phase-B workgroup walks, its grid x."""
    assert Dc * R <= 8 * THREADS and 4 * 32 * (R + 2 * Dc) <= LDS_BYTES and 4 * 2 * Dc * R <= LDS_BYTES
    engine = "mfma1" if R <= 32 and Dc <= 32 else ("mfma2" if R <= 32 and Dc <= 64 else "valu")
    DE = (Dc + 1) & ~1
    DP = DE | 1
    RP = (R + 31) & ~31
    nw = 4
    while nw >= 1 and 4 * (2 * DE * RP + 2 * 32 * nw * DP) > LDS_BYTES:
        nw >>= 1
    assert nw >= 1
    nblk = cdiv(N, 32 * nw)
    tiles = 1
    while tiles < 8 and B * cdiv(nblk, 2 * tiles) >= 1024:
        tiles *= 2
    return {"engine": engine, "nw": nw, "tiles": tiles, "grid_x": cdiv(nblk, tiles), "nblk": nblk,
            "lds_out": 4 * (2 * DE * RP + 2 * 32 * nw * DP)}


def root_facts(B, N, R, D):
    S, rows = choose_split(B, N, 256)
    chunks = root_chunks(R, D)
    return {"S": S, "rows": rows, "chunks": chunks, "launches": [root_launch_facts(B, N, R, w) for _, w in chunks]}


def root_route(B, N, R, D):
    f = root_facts(B, N, R, D)
    per = [f"{l['engine']}({w},nw{l['nw']},tiles{l['tiles']})" for (_, w), l in zip(f["chunks"], f["launches"])]
    return f"S{f['S']}x{f['rows']} " + " ".join(per)


def root_K(B, N, R, D):
    """(K of the output, K of rowdot).  A term U[n,d] V[row,d] C[row,rho] of the output passes
      phase A  the sum over the rows of its slice: at most min(rows, N) roundings whatever the order (VALU: a chain of
               fmaf; matrix cores: per-wave partial sums and two levels across the waves -- a sum of n products rounds a
               term at most n times);
      S - 1    additions of the slices' partials (the first lands on 0.f);
      phase B  a sum of 2 Dc products (U T1 and V T2 in one accumulator): at most 2 Dc roundings whatever the order;
      and chunks - 1 additions of the per-chunk results (kernels.bilinear_root).
    rowdot: a chain of Dc fmaf and chunks - 1 additions."""
    f = root_facts(B, N, R, D)
    wmax = max(w for _, w in f["chunks"])
    nch = len(f["chunks"])
    return min(f["rows"], N) + (f["S"] - 1) + 2 * wmax + (nch - 1), wmax + nch - 1


@functools.lru_cache(maxsize=None)
def root_inputs(case):
    B, N, R, D = case
    g = _rng(4300 + 7 * N + 3 * R + D)
    Cm, U, V = _normal(g, B, N, R), _normal(g, B, N, D), _normal(g, B, N, D)
    C64, U64, V64 = Cm.astype(f64), U.astype(f64), V.astype(f64)
    ref = orc.bilinear_derivative_root(C64, U64, V64)
    mag = orc.bilinear_derivative_root(np.abs(C64), np.abs(U64), np.abs(V64))
    rd = orc.bilinear_derivative_diag(U64, V64)
    rd_mag = orc.bilinear_derivative_diag(np.abs(U64), np.abs(V64))
    return Cm, U, V, ref, mag, rd, rd_mag


# ---- Kronecker: (sum_d U_d K2 V_d^T, sum_d U_d^T K1 V_d) ---------------------------------------------------------------
# (B, n1, n2, D); the label lists the four GEMM stages as name:MxNxK@grid
KRON_CASES = (
    ((2, 1, 7, 1), "T:1x7x7@1x1x2 dK1:1x1x7@1x1x2 S:1x7x1@1x1x2 dK2:7x7x1@1x1x2"),                # n1 = 1
    ((2, 7, 1, 3), "T:7x1x1@1x1x6 dK1:7x7x3@1x1x2 S:7x3x7@1x1x2 dK2:1x1x7@1x1x2"),                # n2 = 1
    ((2, 63, 65, 3), "T:63x65x65@2x1x6 dK1:63x63x195@1x1x2 S:63x195x63@4x1x2 dK2:65x65x63@2x2x2"),  # straddle a tile
    ((1, 64, 64, 17), "T:64x64x64@1x1x17 dK1:64x64x1088@1x1x1 S:64x1088x64@17x1x1 dK2:64x64x64@1x1x1"),  # exact tiles
    ((3, 65, 17, 2), "T:65x17x17@1x2x6 dK1:65x65x34@2x2x3 S:65x34x65@1x2x3 dK2:17x17x65@1x1x3"),  # n1 one above a tile
    ((2, 16, 80, 1), "T:16x80x80@2x1x2 dK1:16x16x80@1x1x2 S:16x80x16@2x1x2 dK2:80x80x16@2x2x2"),  # long K
)


def kron_stages(B, n1, n2, D):
    """kron_bilinear (csrc/lo_kron.hip): (name, M, N, K, grid (x, y, z)) of its four k_gemm stages; the last one runs
    once per column d, accumulating from the second on."""
    def stage(name, M, N, K, z):
        return name, M, N, K, (cdiv(N, GEMM_TILE), cdiv(M, GEMM_TILE), z)
    return (stage("T", n1, n2, n2, B * D), stage("dK1", n1, n1, n2 * D, B), stage("S", n1, n2 * D, n1, B),
            stage("dK2", n2, n2, n1, B))


def kron_route(B, n1, n2, D):
    return " ".join(f"{n}:{M}x{N}x{K}@{g[0]}x{g[1]}x{g[2]}" for n, M, N, K, g in kron_stages(B, n1, n2, D))


def kron_K(B, n1, n2, D):
    """k_gemm is a chain of K fmaf per output (the zero padding of the last 16-slab adds exact zeros).
    dK1 = U T^T: n2 roundings in T = V K2^T, then a chain over (j2, d) of n2 D: n2 + n2 D.
    dK2 = sum_d U_d^T S_d: n1 roundings in S = K1 V, a chain of n1 per column, and D - 1 accumulating launches that add
    with one rounding each: 2 n1 + D - 1."""
    return n2 + n2 * D, 2 * n1 + D - 1


@functools.lru_cache(maxsize=None)
def kron_inputs(case):
    B, n1, n2, D = case
    g = _rng(4400 + 7 * n1 + 3 * n2 + D)
    K1, K2 = _normal(g, B, n1, n1), _normal(g, B, n2, n2)  # not symmetric
    U, V = _normal(g, B, n1 * n2, D), _normal(g, B, n1 * n2, D)
    a = [t.astype(f64) for t in (K1, K2, U, V)]
    ref = orc.bilinear_derivative_kron(*a)
    mag = orc.bilinear_derivative_kron(*[np.abs(t) for t in a])
    # the same contraction with the OTHER factor transposed: what a kernel that read K2 (K1) the wrong way round gives
    swapped = (orc.bilinear_derivative_kron(a[0], np.swapaxes(a[1], -1, -2), a[2], a[3])[0],
               orc.bilinear_derivative_kron(np.swapaxes(a[0], -1, -2), a[1], a[2], a[3])[1])
    return K1, K2, U, V, ref, mag, swapped


# ---- float32 emulation of the kernels' summation orders --------------------------------------------------------------
def fma(a, b, acc):
    """fmaf, vectorised: float32(float64(acc) + float64(a) float64(b)) (the product of two floats is exact in fp64)."""
    return (np.asarray(acc, f64) + np.asarray(a, f64) * np.asarray(b, f64)).astype(f32)


def emu_dense(U, V):
    B, N, D = U.shape
    out = None
    for d0 in range(0, D, BD_MAXD):
        acc = np.zeros((B, N, N), f32)
        for d in range(d0, min(D, d0 + BD_MAXD)):
            acc = fma(U[:, :, None, d], V[:, None, :, d], acc)
        out = acc if out is None else out + acc
    assert out.dtype == f32
    return out


def emu_diag(U, V, constant):
    B, N, D = U.shape
    prod = U * V
    acc = prod[..., 0]
    for d in range(1, D):
        acc = acc + prod[..., d]
    assert acc.dtype == f32
    if not constant:
        return acc
    # k_bil_sum_rows: thread t sums rows t, t + 256, ..; wave_sum (xor butterfly 32 .. 1); (r0 + r1) + (r2 + r3)
    strides = cdiv(N, THREADS)
    padded = np.zeros((B, strides * THREADS), f32)
    padded[:, :N] = acc
    padded = padded.reshape(B, strides, THREADS)
    t = padded[:, 0]
    for s in range(1, strides):
        t = t + padded[:, s]
    w = t.reshape(B, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    r = w[..., 0]
    out = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    assert out.dtype == f32
    return out[:, None]


def emu_root(Cm, U, V):
    """(out, rowdot) of kernels.bilinear_root.  Both phases as sequential fmaf chains: over the rows of a slice in
    phase A (the order of k_bil_root_t; the matrix-core engines' order inside an instruction is not documented), over
    the k pairs of U T1 then V T2 in phase B."""
    B, N, R = Cm.shape
    S, rows = choose_split(B, N, 256)
    out, rowdot = None, None
    for d0, w in root_chunks(R, U.shape[-1]):
        Uc, Vc = U[..., d0:d0 + w], V[..., d0:d0 + w]
        T1, T2 = None, None
        for s in range(S):
            a1, a2 = np.zeros((B, w, R), f32), np.zeros((B, w, R), f32)
            for row in range(s * rows, min(N, (s + 1) * rows)):
                a1 = fma(Vc[:, row, :, None], Cm[:, row, None, :], a1)
                a2 = fma(Uc[:, row, :, None], Cm[:, row, None, :], a2)
            T1, T2 = (a1, a2) if T1 is None else (T1 + a1, T2 + a2)
        acc = np.zeros((B, N, R), f32)
        for k in range(0, w, 2):
            for W, T in ((Uc, T1), (Vc, T2)):
                for kk in range(k, min(k + 2, w)):
                    acc = fma(W[:, :, kk, None], T[:, None, kk, :], acc)
        dot = np.zeros((B, N), f32)
        for d in range(w):
            dot = fma(Uc[..., d], Vc[..., d], dot)
        out, rowdot = (acc, dot) if out is None else (out + acc, rowdot + dot)
    assert out.dtype == f32 and rowdot.dtype == f32
    return out, rowdot


def emu_kron(K1, K2, U, V):
    B, n1, n2 = K1.shape[0], K1.shape[-1], K2.shape[-1]
    D = U.shape[-1]
    Ur, Vr = U.reshape(B, n1, n2, D), V.reshape(B, n1, n2, D)
    T = np.zeros((B, n1, n2, D), f32)   # T[i1, j2, d] = sum_i2 V[i1, i2, d] K2[j2, i2]
    for i2 in range(n2):
        T = fma(Vr[:, :, i2, None, :], K2[:, None, :, i2, None], T)
    Uf, Tf = U.reshape(B, n1, n2 * D), T.reshape(B, n1, n2 * D)
    dK1 = np.zeros((B, n1, n1), f32)    # dK1[j1, i1] = sum_k U[j1, k] T[i1, k]
    for k in range(n2 * D):
        dK1 = fma(Uf[:, :, None, k], Tf[:, None, :, k], dK1)
    Sm = np.zeros((B, n1, n2, D), f32)  # S[i1, j2, d] = sum_j1 K1[i1, j1] V[j1, j2, d]
    for j1 in range(n1):
        Sm = fma(K1[:, :, j1, None, None], Vr[:, None, j1], Sm)
    dK2 = None
    for d in range(D):                  # dK2[a, b] (+)= sum_j1 U[j1, a, d] S[j1, b, d]
        acc = np.zeros((B, n2, n2), f32)
        for j1 in range(n1):
            acc = fma(Ur[:, j1, :, None, d], Sm[:, j1, None, :, d], acc)
        dK2 = acc if dK2 is None else dK2 + acc
    assert dK1.dtype == f32 and dK2.dtype == f32
    return dK1, dK2


# ---- SLQ: eigh of the CG / Lanczos tridiagonals, the reference's mask, the log quadrature ----------------------------
SLQ_N = 100
# (P, B, T, kind)
SLQ_CASES = (
    ((1, 1, 1, "spd"), "M1 blocks1 T1 spd"),           # T = 1
    ((5, 13, 2, "spd"), "M65 blocks2 T2 spd"),         # 65 tridiagonals: two thread blocks
    ((3, 2, 31, "spd"), "M6 blocks1 T31 spd"),         # T one below the maximum
    ((2, 3, 32, "spd"), "M6 blocks1 T32 spd"),         # T at the maximum
    ((2, 2, 20, "padded"), "M4 blocks1 T20 padded"),   # identity padding after step 7
    ((2, 2, 12, "negative"), "M4 blocks1 T12 negative"),  # a negative eigenvalue
    ((1, 2, 8, "repeated"), "M2 blocks1 T8 repeated"),    # repeated eigenvalues
)
SLQ_PAD_FROM = 7


def slq_route(P, B, T, kind):
    assert T <= EIG_MAX_T
    return f"M{P * B} blocks{cdiv(P * B, 64)} T{T} {kind}"


@functools.lru_cache(maxsize=None)
def slq_matrices(case):
    """t_mat [P, B, T, T] float32.  spd: alpha in [1, 2], beta in [0, 0.4] (diagonally dominant: every eigenvalue is
    >= 0.2).  padded: alpha = 1 and beta = 0 from step 7 on, as an early-converged CG leaves them.  negative: the middle
    diagonal entry of an spd matrix set to -1 -- a rank-one downdate, so exactly one eigenvalue drops (to <= -1, the
    Rayleigh quotient of that unit vector) and by interlacing the others stay >= 0.2.  repeated: 1.5 I."""
    P, B, T, kind = case
    g = _rng(4500 + 7 * T + P)
    alpha = (1.0 + g.random((P, B, T))).astype(f32)
    beta = (0.4 * g.random((P, B, max(T - 1, 0)))).astype(f32)
    if kind == "padded":
        alpha[..., SLQ_PAD_FROM:] = 1.0
        beta[..., SLQ_PAD_FROM - 1:] = 0.0
    elif kind == "negative":
        alpha[..., T // 2] = -1.0
    elif kind == "repeated":
        alpha[:] = 1.5
        beta[:] = 0.0
    else:
        assert kind == "spd"
    t = np.zeros((P, B, T, T), f32)
    i = np.arange(T)
    t[..., i, i] = alpha
    t[..., i[:-1], i[1:]] = beta
    t[..., i[1:], i[:-1]] = beta
    return t


@functools.lru_cache(maxsize=None)
def slq_reference(case):
    """fp64 eigh of the float32-valued matrices with the reference's mask (utils/lanczos.py:185-187): raw eigenvalues
    lam [P,B,T], mask, masked eigenvalues, the projection of the matrix on its non-negative eigenspace [P,B,T,T],
    logdet [B] and its magnitude (n / P) sum w0^2 |log lambda|."""
    P = case[0]
    lam, vec = np.linalg.eigh(slq_matrices(case).astype(f64))
    mask = lam >= 0
    ev = np.where(mask, lam, 1.0)
    vm = vec * mask[..., None, :]
    proj = (vm * ev[..., None, :]) @ np.swapaxes(vm, -1, -2)
    w0sq = vm[..., 0, :] ** 2
    logdet = SLQ_N / P * (w0sq * np.log(ev)).sum(-1).sum(0)
    logdet_mag = SLQ_N / P * (w0sq * np.abs(np.log(ev))).sum(-1).sum(0)
    return {"lam": lam, "mask": mask, "evals": ev, "proj": proj, "logdet": logdet, "logdet_mag": logdet_mag}


def slq_check(case, evals, evecs, logdet):
    """The SLQ checks on float32 results (evecs / logdet may be None).  Returns {name: err / bound} -- every entry must
    be <= 1 -- and asserts what has to be exact: a masked eigenvalue is 1.0, its eigenvector column 0.0.
      evals   |l - l64| <= 2^-23 max |l64|: fp64 arithmetic and one rounding to float32 (2^-24 |l|), the same again
              for the fp64 iteration's own error;
      recon   |V L V^T - proj| <= (2T + 1) 2^-24 max |l64|: each of the T terms v_ik l_k v_jk carries three rounded
              factors and sum_k |v_ik v_jk| <= 1, so 3 u max |l| would do;
      orth    |V^T V - I| <= (2T + 1) 2^-24 on the unmasked columns (two rounded factors per term);
      logdet  |ld - ld64| <= 2^-23 (n / P) sum w0^2 |log l|.
    Not column by column: signs, and with repeated eigenvalues the basis, are free."""
    T = case[2]
    r = slq_reference(case)
    lmax = np.abs(r["lam"]).max(-1)  # [P, B]
    masked = ~r["mask"]
    evals = np.asarray(evals)
    assert evals.dtype == f32 and evals.shape == r["lam"].shape
    assert (evals[masked] == f32(1.0)).all(), "a masked eigenvalue is not exactly 1"
    out = {"evals": float((np.abs(evals.astype(f64) - r["evals"]) / (2.0 ** -23 * lmax[..., None])).max())}
    if evecs is not None:
        evecs = np.asarray(evecs)
        assert evecs.dtype == f32 and evecs.shape == r["proj"].shape
        assert (evecs[np.broadcast_to(masked[..., None, :], evecs.shape)] == 0).all(), "a masked column is not exactly 0"
        v = evecs.astype(f64)
        lam_out = np.where(masked, 0.0, evals.astype(f64))
        recon = (v * lam_out[..., None, :]) @ np.swapaxes(v, -1, -2)
        bound = (2 * T + 1) * U24
        out["recon"] = float((np.abs(recon - r["proj"]) / (bound * lmax[..., None, None])).max())
        eye = np.eye(T) * r["mask"][..., None, :]
        out["orth"] = float((np.abs(np.swapaxes(v, -1, -2) @ v - eye) / bound).max())
    if logdet is not None:
        logdet = np.asarray(logdet)
        assert logdet.dtype == f32 and logdet.shape == r["logdet"].shape
        err = np.abs(logdet.astype(f64) - r["logdet"])
        bound = 2.0 ** -23 * r["logdet_mag"]
        assert (err[bound == 0] == 0).all()
        out["logdet"] = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return out


def ql_implicit64(t):
    """Eigenvalues (ascending) and eigenvectors of one symmetric tridiagonal matrix by the implicit-shift QL iteration
    in fp64 (Wilkinson & Reinsch, Handbook for Automatic Computation II/3, `imtql2`): a reference of its own, written
    from the algorithm, not the code under test."""
    n = t.shape[-1]
    d = np.array(np.diagonal(t), f64)
    e = np.zeros(n, f64)
    e[:n - 1] = np.diagonal(t, 1)
    z = np.eye(n)
    eps = np.finfo(f64).eps
    for l in range(n):
        for sweep in range(100):
            m = l
            while m < n - 1 and abs(e[m]) > eps * (abs(d[m]) + abs(d[m + 1])):
                m += 1
            if m == l:
                break
            g = (d[l + 1] - d[l]) / (2.0 * e[l])
            r = np.hypot(g, 1.0)
            g = d[m] - d[l] + e[l] / (g + np.copysign(r, g))
            s, c, p = 1.0, 1.0, 0.0
            underflow = False
            for i in range(m - 1, l - 1, -1):
                f, b = s * e[i], c * e[i]
                r = np.hypot(f, g)
                e[i + 1] = r
                if r == 0.0:
                    d[i + 1] -= p
                    e[m] = 0.0
                    underflow = True
                    break
                s, c = f / r, g / r
                g = d[i + 1] - p
                r = (d[i] - g) * s + 2.0 * c * b
                p = s * r
                d[i + 1] = g + p
                g = c * r - b
                zi, zi1 = z[:, i].copy(), z[:, i + 1].copy()
                z[:, i + 1] = s * zi + c * zi1
                z[:, i] = c * zi - s * zi1
            if underflow:
                continue
            d[l] -= p
            e[l] = g
            e[m] = 0.0
        else:
            raise RuntimeError("QL did not converge")
    order = np.argsort(d, kind="stable")
    return d[order], z[:, order]


def slq_from_eigh64(case, lam, vec):
    """What an exact-to-fp64 solver hands back after the mask and ONE rounding to float32: (evals, evecs, logdet)."""
    P = case[0]
    mask = lam >= 0
    ev = np.where(mask, lam, 1.0)
    vm = vec * mask[..., None, :]
    logdet = SLQ_N / P * (vm[..., 0, :] ** 2 * np.log(ev)).sum(-1).sum(0)
    return ev.astype(f32), vm.astype(f32), logdet.astype(f32)
