"""Edge cases of the Kronecker matvec y = (K1 (x) K2) v + d o v behind lo_matvec_f32 (csrc/lo_kron.hip) and lo_matvec_f64
(k64_kron_gemm, csrc/lo_matvec_f64.hip), shared by tests/test_kron_edges_cpu.py (the tables' own preconditions, no GPU)
and tests/test_gpu_kron_edges.py (the kernels against the references below).  Everything here is numpy: restatements of
the host-side launch arithmetic, a `route(case)` that says which engine, which template instantiation and which named
edges a case sits on, the case tables, the inputs and the references.  Not a test module.

Every engine is sums of products.  The entries of K1, K2 and v are integers from {+-1, +-2, +-3} (never 0) and the
diagonal holds 1, 2 or 3, so every product and every partial sum is an integer and |y| <= 27 n1 n2 + 9.  Every case keeps
that below 2^24, so float32 is exact in any summation order, with or without fmaf, on the vector ALU and on the fp32
matrix cores (v_mfma_f32_32x32x2_f32).  The kernels must return the reference bit for bit.  The reference is
K1 V K2^T + d o V in numpy float64 (exact below 2^53; an int64 matmul is too slow at the fused sizes), and
tests/test_kron_edges_cpu.py compares it with an int64 einsum on the small shapes.

K1 and K2 are NOT symmetric: both matrix-core GEMMs are in the "NT" form and the second VALU pass reads K2 with strides
(1, n2), so a factor read transposed is the likeliest mistake, and symmetric factors cannot see it.  Each case carries
the two references with one factor transposed; the kernels' result must differ from both."""
import functools
from dataclasses import dataclass

import numpy as np

# ---- restated launch arithmetic (csrc/lo_kron.hip unless said otherwise) -----------------------------------------------
THREADS = 256                       # kThreads (lo_internal.h:11)
BM, BN, BK = 64, 64, 16             # k_gemm's tile (lo_kron.hip:33)
KM_BM, KM_BN, KM_BK = 128, 128, 64  # k_kron_nt_mfma's tile (lo_kron.hip:106)
FUSED_GATE = 96                     # `B * (n2 / KM_BN) >= 96` (lo_kron.hip:487)
COLS_MAX = 64                       # kron_mfma_cols_ok: c <= 64 (lo_kron.hip:561)
GRID_Z_MAX = 65535                  # `B * c > 65535` is refused (lo_kron.hip:616)
PLAN_TAIL = 256                     # kPlanTail (lo_internal.h:383)
F64_TAIL = 1024                     # kMv64Tail (lo_matvec_f64.hip:390)
GT, GK = 32, 16                     # kGT, kGK of k64_kron_gemm (lo_matvec_f64.hip:232)
LIMIT = 1 << 24                     # below it every float32 integer sum is exact
CAP_BYTES = 128 << 20               # a case's device footprint: operands + y + workspace
DIAG_MODES = ("none", "full", "const")


def ceil_div(a, b):
    return -(-a // b)


def kron_mfma_ok(n1, n2, c):
    """kron_mfma_ok (lo_kron.hip:468)."""
    return c == 1 and n1 % 4 == 0 and n2 % 4 == 0 and n1 >= 64 and n2 >= 64


def kron_mfma_cols_ok(n1, n2, c):
    """kron_mfma_cols_ok (lo_kron.hip:561)."""
    return 1 < c <= COLS_MAX and kron_mfma_ok(n1, n2, 1)


def kron_fused_ok(n1, n2, no_fused=False):
    """kron_fused_ok (lo_kron.hip:461); `no_fused`: LO_NO_KRON_FUSED is set (read by getenv at every call)."""
    return n1 in (128, 256) and n2 % 128 == 0 and n2 >= 128 and not no_fused


def kron_fused_taken(B, n1, n2, no_fused=False):
    """The gate of kron_matvec_mfma (lo_kron.hip:487)."""
    return kron_fused_ok(n1, n2, no_fused) and B * (n2 // KM_BN) >= FUSED_GATE


def km_aligned(n1, n2):
    """km_aligned (lo_kron.hip:465): the unguarded instantiation."""
    return n1 % 128 == 0 and n2 % 128 == 0


def km_tiles(M, N):
    return ceil_div(M, KM_BM) * ceil_div(N, KM_BN)


def kron_S_dot(n1, n2, c, S_default):
    """kron_S_dot (lo_kron.hip:469): the dot partials per member the matrix-core epilogues write."""
    return km_tiles(n1, n2) if kron_mfma_ok(n1, n2, c) else S_default


def gemm_grid(M, N, nbatch):
    """launch_gemm (lo_kron.hip:96)."""
    return (ceil_div(N, BN), ceil_div(M, BM), nbatch)


def km_grid(M, N, Z):
    """km_launch (lo_kron.hip:475-476): whole rounds of the 8 XCDs times the tiles of a member."""
    return ceil_div(Z, 8) * 8 * km_tiles(M, N)


def fused_grid(B, n2):
    """The fused launch (lo_kron.hip:491)."""
    return ceil_div(B, 8) * 8 * (n2 // KM_BN)


def fused_inst(n1, n2):
    """<NI, NS> of k_kron_fused (lo_kron.hip:493-496)."""
    if n1 == 256:
        return (8, 4) if n2 == 256 else (8, 0)
    return (4, 2) if n2 == 128 else (4, 0)


def cols_grid(B, N):
    """k_kron_cols (lo_kron.hip:569)."""
    return (ceil_div(N, THREADS), B)


def cols_lds_bytes(c):
    """The dynamic LDS of k_kron_cols (lo_kron.hip:568): 256 rows of c | 1 floats."""
    return 4 * THREADS * (c | 1)


def kron_workspace_floats(B, n1, n2, c):
    """kron_plan (lo_matvec.hip:63-69): one buffer of B N c floats, two on the many-column route."""
    return B * n1 * n2 * c * (2 if kron_mfma_cols_ok(n1, n2, c) else 1)


def f64_grids(B, n1, n2, c):
    """The two launches of kron_run (lo_matvec_f64.hip:371, 380) and kfast = mfast = (c < 8) (:369)."""
    return {"pass1": (ceil_div(n1 * c, GT), ceil_div(n2, GT), B), "pass2": (ceil_div(n2 * c, GT), ceil_div(n1, GT), B),
            "kfast": c < 8}


def choose_split(B, N, min_rows=256, max_split=256):
    """choose_split (lo_vec.hip:14) -> (S, rows per slice)."""
    S = ceil_div(1024, B)
    maxS = max(1, N // max(min_rows, 4))
    S = max(1, min(S, maxS))
    cap = 64
    while cap < max_split and (cap * 2) * (cap * 2) * 16 <= N:
        cap *= 2
    S = min(S, min(cap, max_split))
    rows = ceil_div(ceil_div(N, S), 4) * 4
    return ceil_div(N, rows), rows


# ---- the cases -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Kron:
    group: str            # the table the case is listed in (the parametrised GPU test it runs in)
    n1: int
    n2: int
    c: int
    B: int
    diag: str
    f64: bool = False

    @property
    def N(self):
        return self.n1 * self.n2

    @property
    def id(self):
        return f"{self.n1}x{self.n2}-c{self.c}-B{self.B}-{self.diag}"

    @property
    def bound(self):
        return 27 * self.n1 * self.n2 + 9

    @property
    def itemsize(self):
        return 8 if self.f64 else 4

    @property
    def workspace_bytes(self):
        """What lo_matvec_workspace_bytes / lo_matvec_f64_workspace_bytes report (the take starts the arena: no padding)."""
        if self.f64:
            return F64_TAIL + 8 * self.B * self.N * self.c      # kron_layout (lo_matvec_f64.hip:356)
        return PLAN_TAIL + 4 * kron_workspace_floats(self.B, self.n1, self.n2, self.c)

    @property
    def footprint(self):
        """Device bytes of K1, K2, v, y, the diagonal and the workspace."""
        d = {"none": 0, "full": self.B * self.N, "const": self.B}[self.diag]
        operands = self.B * (self.n1 ** 2 + self.n2 ** 2) + 2 * self.B * self.N * self.c + d
        return self.itemsize * operands + self.workspace_bytes


_MODE = {"n": "none", "f": "full", "c": "const"}


def _rows(group, rows, f64=False):
    """rows of (n1, n2, c, B, modes) with modes a string over n / f / c."""
    return tuple(Kron(group, n1, n2, c, B, _MODE[m], f64) for n1, n2, c, B, modes in rows for m in modes)


# 1. the strided VALU GEMM k_gemm: whatever kron_mfma_ok and kron_mfma_cols_ok refuse
VALU = _rows("valu", (
    (1, 1, 1, 1, "nf"),        # one element: sb_c == 1, sa_c == 1
    (15, 1, 2, 3, "c"),        # sb_c == 1 with inner = 2
    (16, 13, 5, 1, "f"),       # n2 c = 65, whole BK slabs in pass 1
    (17, 17, 1, 3, "nc"),      # one step past a BK slab in both passes
    (63, 63, 1, 1, "f"),       # n2 c = 63
    (17, 32, 2, 1, "c"),       # n2 c = 64
    (65, 65, 1, 3, "nfc"),     # two row tiles and two column tiles in both passes, n2 c = 65
    (129, 13, 2, 1, "f"),      # three row tiles, the last of one row
    (1, 66, 5, 1, "c"),        # M = 1 with six column tiles in pass 1, two in pass 2
    (63, 17, 5, 3, "n"),
    (65, 63, 2, 1, "fc"),      # two row tiles with inner = 2
    (129, 65, 1, 1, "n"),
    (16, 66, 2, 3, "f"),
    (15, 63, 5, 1, "c"),
    (64, 64, 65, 1, "nf"),     # c > 64 on factors the matrix cores would take: 65 column tiles in pass 1
    (68, 64, 65, 1, "c"),      # ... with two row tiles
    (65, 68, 1, 1, "f"),       # n1 refused by kron_mfma_ok
    (65, 68, 1, 3, "n"),
    (64, 66, 1, 1, "c"),       # n2 refused
))

# 2. k_kron_nt_mfma, two launches, one column: aligned {128, 256, 384}^2 below the fused gate (or n1 = 384), guarded
#    sizes one step past / before a tile or a slab, mixed aligned / ragged pairs; B = 1, 7, 8, 9 on both
MFMA = _rows("mfma", (
    (128, 128, 1, 1, "nf"), (128, 256, 1, 7, "c"), (128, 384, 1, 9, "f"), (256, 128, 1, 8, "n"), (256, 256, 1, 9, "fc"),
    (256, 384, 1, 1, "c"), (384, 128, 1, 7, "f"), (384, 256, 1, 8, "c"), (384, 384, 1, 9, "nf"),
    (64, 64, 1, 1, "nfc"), (68, 68, 1, 7, "nfc"), (260, 132, 1, 9, "fc"), (132, 260, 1, 8, "n"), (124, 252, 1, 7, "f"),
    (252, 124, 1, 1, "c"), (192, 64, 1, 8, "f"), (64, 192, 1, 9, "n"), (252, 260, 1, 1, "f"),
    (128, 68, 1, 7, "fc"), (68, 128, 1, 9, "nf"), (256, 132, 1, 8, "c"),
))

# 3. the many-column route k_kron_cols -> two matrix-core GEMMs with a_div = c -> k_kron_cols; every shape with every
#    diagonal mode (39 cases: within the table limit, so nothing is thinned out)
COLS = _rows("cols", (
    (64, 64, 2, 1, "nfc"), (64, 64, 3, 1, "nfc"), (64, 64, 16, 1, "nfc"), (64, 64, 17, 1, "nfc"), (64, 64, 63, 1, "nfc"),
    (64, 64, 64, 1, "nfc"),      # 66 560 bytes of dynamic LDS
    (64, 64, 2, 4, "nfc"),         # B c = 8
    (64, 68, 3, 3, "nfc"),        # B c = 9, N = 4352 = 17 * 256
    (64, 68, 17, 1, "nfc"),
    (68, 68, 3, 1, "nfc"),        # B c = 3, N = 4624: a last block of 16 rows
    (68, 68, 17, 3, "nfc"),       # B c = 51
    (128, 128, 3, 1, "nfc"),      # aligned: no guard
    (128, 128, 17, 1, "nfc"),
))

# 4. k_kron_fused<NI, NS> at the gate's boundary and at B that is no multiple of 8 (128 (x) 128 at B = 95: two launches);
#    every shape with every diagonal mode
FUSED = _rows("fused", (
    (128, 128, 1, 96, "nfc"), (128, 128, 1, 97, "nfc"), (128, 128, 1, 95, "nfc"),
    (128, 256, 1, 48, "nfc"), (128, 256, 1, 49, "nfc"), (128, 384, 1, 32, "nfc"),
    (256, 256, 1, 48, "nfc"), (256, 256, 1, 49, "nfc"),
    (256, 128, 1, 96, "nfc"), (256, 384, 1, 32, "nfc"),
))

# 5. float64: k64_kron_gemm, both passes
F64 = _rows("f64", (
    (1, 1, 1, 1, "nfc"), (15, 17, 2, 3, "nfc"), (16, 33, 2, 1, "nfc"), (31, 32, 1, 3, "nfc"), (33, 31, 1, 1, "nfc"),
    (32, 16, 7, 1, "nfc"), (17, 15, 8, 3, "nfc"), (65, 1, 9, 1, "nfc"), (1, 65, 7, 3, "nfc"), (32, 32, 8, 1, "nfc"),
    (33, 33, 9, 1, "nfc"), (16, 65, 2, 1, "nfc"), (65, 65, 1, 1, "nfc"),
), f64=True)

TABLES = {"valu": VALU, "mfma": MFMA, "cols": COLS, "fused": FUSED, "f64": F64}
ALL = VALU + MFMA + COLS + FUSED + F64

# the float64 sum of two Kronecker terms and one diagonal: the second term runs with accumulate = 1
SUM_B, SUM_TERMS, SUM_COLS = 3, ((17, 33), (33, 17)), (1, 9)
# the refused VALU shape: B c = 65552 > 65535 on 1 (x) 1
REFUSED = Kron("refused", 1, 1, 17, 3856, "none")
# one case per float32 engine on operands that start 4 bytes off a 16-byte boundary
MISALIGNED = (Kron("mfma", 128, 256, 1, 3, "full"), Kron("mfma", 68, 132, 1, 3, "const"), Kron("cols", 64, 68, 3, 3, "full"),
              Kron("fused", 128, 128, 1, 97, "full"), Kron("valu", 65, 65, 2, 3, "const"))
# one CG step: (n1, n2, B) on the aligned, guarded and fused routes
CG_STEP = ((128, 256, 3), (68, 132, 3), (260, 64, 9), (128, 128, 97))


# ---- route(case) -----------------------------------------------------------------------------------------------------------
def _past(n, step):
    return n % step == 4


def _before(n, step):
    return n % step == step - 4


def _mfma_edges(k, Z):
    n1, n2 = k.n1, k.n2
    e = {"aligned" if km_aligned(n1, n2) else "guard", f"diag {k.diag}"}
    if km_tiles(n1, n2) > 1:
        e.add("tiles > 1")
    if ceil_div(n1, KM_BM) > 1 and ceil_div(n2, KM_BN) > 1:
        e.add("tiles in both directions")
    for n in (n1, n2):
        if n % KM_BK:
            e.add("ragged K slab")
        if _past(n, KM_BM):
            e.add("one step past a tile")
        if _before(n, KM_BM):
            e.add("one step before a tile")
        if _past(n, KM_BK) and not _past(n, KM_BM):
            e.add("one step past a slab")
        if n == 64:
            e.add("half a tile")
    if (n1 % 128 == 0) != (n2 % 128 == 0):
        e.add("mixed aligned / ragged")
    e.add("Z % 8 != 0" if Z % 8 else "Z % 8 == 0")
    e.add("Z < 8" if Z < 8 else "Z == 8" if Z == 8 else "Z > 8")
    return e


def route(k, no_fused=False):
    """{"engine", "inst" (template instantiations), "edges" (names), "kernels" ({profiler name: launches}), "grids",
    "workspace" (bytes without the tail)}: what serves a case.  `no_fused`: LO_NO_KRON_FUSED is set."""
    B, n1, n2, c = k.B, k.n1, k.n2, k.c
    out = {"workspace": k.workspace_bytes - (F64_TAIL if k.f64 else PLAN_TAIL)}
    if k.f64:   # k64_kron_gemm has no profiler scope: a float64 call reports no kernel
        g = f64_grids(B, n1, n2, c)
        e = {"kfast" if g["kfast"] else "kslow", f"diag {k.diag}", f"c = {c}"}
        for name, Q in (("pass 1", n1 * c), ("pass 2", n2 * c)):
            if Q in (31, 32, 33):
                e.add(f"Q = {Q}")
            if Q > GT:
                e.add(f"{name}: q tiles > 1")
        for n in (n1, n2):
            if n in (31, 32, 33):
                e.add(f"n = {n}")
            if n > GT:
                e.add("m tiles > 1")
            if n % GK:
                e.add("ragged kGK slab")
            if n == 1:
                e.add("n = 1")
        return dict(out, engine="f64", inst={("k64_kron_gemm", g["kfast"])}, edges=e, kernels={}, grids=g)
    if kron_mfma_ok(n1, n2, c):
        if kron_fused_taken(B, n1, n2, no_fused):
            inst = fused_inst(n1, n2)
            e = {f"diag {k.diag}", "B % 8 != 0" if B % 8 else "B % 8 == 0"}
            if B * (n2 // KM_BN) in (FUSED_GATE, FUSED_GATE + 1):
                e.add("at the gate")
            if inst[1] == 0:
                e.add(f"NS = 0 at n2 = {n2}")
            return dict(out, engine="fused", inst={("k_kron_fused",) + inst}, edges=e, kernels={"kron_fused": 1},
                        grids={"fused": fused_grid(B, n2)})
        e = _mfma_edges(k, B)
        if kron_fused_ok(n1, n2) and not no_fused:
            e.add("below the gate")
        guard = not km_aligned(n1, n2)
        return dict(out, engine="mfma", inst={("k_kron_nt_mfma", False, guard), ("k_kron_nt_mfma", True, guard)}, edges=e,
                    kernels={"kron_gemm_mfma": 2}, grids={"pass1": km_grid(n2, n1, B), "pass2": km_grid(n1, n2, B)})
    if kron_mfma_cols_ok(n1, n2, c):
        e = _mfma_edges(k, B * c) - {f"diag {k.diag}"}
        e |= {f"cols diag {k.diag}", "ld = c" if c & 1 else "ld = c + 1", f"c = {c}"}
        if cols_lds_bytes(c) > 65536:
            e.add("LDS > 64 KB")
        if k.N % THREADS:
            e.add("ragged last block")
        if B > 1:
            e.add("a_div with B > 1")
        return dict(out, engine="cols", inst={("k_kron_cols",), ("k_kron_nt_mfma", False, not km_aligned(n1, n2))}, edges=e,
                    kernels={"kron_cols": 2, "kron_gemm_mfma": 2},
                    grids={"cols": cols_grid(B, k.N), "lds": cols_lds_bytes(c), "gemm": km_grid(n1, n2, B * c)})
    # k_gemm twice (lo_kron.hip:597-618), then vec_add_diag (lo_matvec.hip:85) where there is a diagonal
    g1, g2 = gemm_grid(n1, n2 * c, B), gemm_grid(n1, n2, B * c)
    e = {f"diag {k.diag}", "p2 sa_c == 1" if c == 1 else "p2 sa_c != 1", f"B = {B}"}
    if g1[1] > 1:
        e.add("row tiles > 1")
    if g1[0] > 1:
        e.add("p1 column tiles > 1")
    if g2[0] > 1:
        e.add("p2 column tiles > 1")
    if n1 % BK:
        e.add("p1 ragged BK slab")
    if n2 % BK:
        e.add("p2 ragged BK slab")
    if n2 * c in (63, 64, 65):
        e.add(f"n2 c = {n2 * c}")
    if n2 == 1:
        e.add("sb_c == 1")
    if c > 1:
        e.add("inner > 1")
    if c > COLS_MAX and kron_mfma_ok(n1, n2, 1):
        e.add("c > 64 on matrix-core factors")
    if c == 1 and min(n1, n2) >= 64 and (n1 % 4 == 0) != (n2 % 4 == 0):
        e.add("one factor refused by kron_mfma_ok")
    kernels = {"kron_gemm": 2}
    if k.diag != "none":
        kernels["vec_add_diag"] = 1
    return dict(out, engine="valu", inst={("k_gemm",)}, edges=e, kernels=kernels, grids={"pass1": g1, "pass2": g2},
                refused=B * c > GRID_Z_MAX)


# ---- inputs and references -------------------------------------------------------------------------------------------------
INTS = np.array([-3, -2, -1, 1, 2, 3], np.float32)


def rng(*key):
    return np.random.Generator(np.random.PCG64([5400, *key]))


def ints(r, shape):
    return INTS[r.integers(0, 6, size=shape, dtype=np.int8)]


def factor(r, B, n):
    """[B, n, n] of non-zero integers with K[n - 1, 0] = -K[0, n - 1] in every member: never symmetric for n > 1."""
    K = ints(r, (B, n, n))
    if n > 1:
        K[:, n - 1, 0] = -K[:, 0, n - 1]
    return K


def const_diag(B):
    """One of 1, 2, 3 per member, neighbours different: what LO_DIAG_CONST reads at dd[b]."""
    return (np.arange(B) % 3 + 1).astype(np.float32)


def product(K1, K2, v):
    """K1 V K2^T in float64 for V = v viewed as [B, n1, n2, c]: two batched GEMMs, every value an integer below 2^53."""
    B, n1, n2 = K1.shape[0], K1.shape[-1], K2.shape[-1]
    c = v.shape[-1]
    K1, K2, v = (np.asarray(a, np.float64) for a in (K1, K2, v))
    W = (K1 @ v.reshape(B, n1, n2 * c)).reshape(B, n1, n2, c)
    Y = W.transpose(0, 1, 3, 2).reshape(B, n1 * c, n2) @ K2.transpose(0, 2, 1)
    return np.ascontiguousarray(Y.reshape(B, n1, c, n2).transpose(0, 1, 3, 2)).reshape(B, n1 * n2, c)


def product_int64(K1, K2, v):
    """The same by an int64 einsum (small shapes only)."""
    B, n1, n2 = K1.shape[0], K1.shape[-1], K2.shape[-1]
    V = v.astype(np.int64).reshape(B, n1, n2, v.shape[-1])
    W = np.einsum("bij,bjlc->bilc", K1.astype(np.int64), V)
    return np.einsum("bilc,bkl->bikc", W, K2.astype(np.int64)).reshape(B, n1 * n2, -1)


def _frozen(data):
    for a in data.values():
        a.setflags(write=False)
    return data


@functools.lru_cache(maxsize=2)
def data(B, n1, n2, c, seed=0):
    """{K1 [B, n1, n1], K2 [B, n2, n2], v [B, N, c], d_full [B, N], d_const [B], Kv, Kv_t1, Kv_t2 (float64: the product,
    the product with K1 transposed, with K2 transposed)} of a shape, as float32 integers; members differ."""
    r = rng(seed, B, n1, n2, c)
    K1, K2, v = factor(r, B, n1), factor(r, B, n2), ints(r, (B, n1 * n2, c))
    return _frozen({"K1": K1, "K2": K2, "v": v, "d_full": r.integers(1, 4, size=(B, n1 * n2)).astype(np.float32),
                    "d_const": const_diag(B), "Kv": product(K1, K2, v),
                    "Kv_t1": product(K1.transpose(0, 2, 1), K2, v), "Kv_t2": product(K1, K2.transpose(0, 2, 1), v)})


def case_data(k):
    return data(k.B, k.n1, k.n2, k.c)


def diag_of(dat, mode):
    return {"none": None, "full": dat["d_full"], "const": dat["d_const"]}[mode]


def diag_term(d, v, mode):
    """d o v in float64 for mode "none" / "full" (d [B, N]) / "const" (d [B])."""
    if mode == "none":
        return 0.0
    d = d.astype(np.float64)
    return (d[:, :, None] if mode == "full" else d[:, None, None]) * v.astype(np.float64)


def reference(k, which="Kv"):
    """The float64 product of a case with its diagonal; which = "Kv_t1" / "Kv_t2": with K1 / K2 transposed."""
    dat = case_data(k)
    return dat[which] + diag_term(diag_of(dat, k.diag), dat["v"], k.diag)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def as_dtype(ref, dtype):
    """The float64 reference in the kernels' element type, which must lose nothing."""
    ref = np.asarray(ref)
    assert ref.dtype == np.float64, ref.dtype
    out = ref.astype(dtype)
    assert np.array_equal(out.astype(np.float64), ref), "the reference is not representable in the kernels' type"
    return out


def exact(got, ref):
    """Whether `got` (float32 or float64, what a kernel returns) IS the float64 array `ref`, element for element."""
    got = np.asarray(got)
    assert got.dtype in (np.float32, np.float64), got.dtype
    r = as_dtype(ref, got.dtype)
    return got.shape == r.shape and np.array_equal(got, r)


def mismatches(got, ref, limit=8):
    """Where and by how much `got` differs from `ref`, for a failing assertion's message."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return f"shape {got.shape} against {ref.shape}"
    bad = np.argwhere(~(got == ref))
    rows = [f"{tuple(int(x) for x in i)}: {float(got[tuple(i)])!r} != {float(ref[tuple(i)])!r}" for i in bad[:limit]]
    return f"{len(bad)} of {got.size} differ; first: " + "; ".join(rows)
