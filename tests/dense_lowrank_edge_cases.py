"""Edge cases of the dense and low-rank matvecs behind lo_matvec_f32 (csrc/lo_dense.hip, lo_dense_mfma.hip, lo_skinny.hip,
lo_skinny_mfma.hip, lo_lowrank_mv.hip), shared by tests/test_dense_lowrank_edges_cpu.py (the tables' own preconditions, no
GPU) and tests/test_gpu_dense_lowrank_edges.py (the kernels against the references below).  Everything here is numpy:
restatements of the host-side launch arithmetic, a `route(case)` that says which kernels and which template
instantiations serve a case, the case tables, the inputs and the references.  Not a test module.

Every kernel of these files is sums of products.  The entries of K, C and v are integers from {+-1, +-2, +-3} (never 0)
and the diagonal holds 1, 2 or 3, so every product and every partial sum is an integer: |y| <= 9 N + 9 for a dense
operator, |C^T v| <= 9 N and |y| <= 27 N R + 9 for a low-rank one.  Every case keeps its bound below 2^24, so float32 is
exact in any summation order, with or without fmaf, on the vector ALU and on the fp32 matrix cores (fmaf chains).  The
kernels must return the int64 reference bit for bit; a dropped, doubled or mis-indexed term moves the result by at
least 1."""
import functools
from dataclasses import dataclass

import numpy as np

# ---- restated launch arithmetic ------------------------------------------------------------------------------------------
THREADS = 256                  # kThreads
DM_ROWS, DM_KB = 64, 128       # lo_dense_mfma.hip: rows of a workgroup tile, k of a slab
MAX_RANK = 256                 # kMaxRank (lo_internal.h)
PLAN_TAIL = 256                # kPlanTail (lo_internal.h)
LR_MIN_ROWS = 256              # the min_rows lo_matvec_f32 and lo_matvec_workspace_bytes pass to choose_split
MV_ROWS = 1024                 # lo_lowrank_mv.hip: rows per workgroup of the resident kernel
LIMIT = 1 << 24                # below it every float32 integer sum is exact
DIAG_MODES = ("none", "full", "const")


def ceil_div(a, b):
    return -(-a // b)


def align256(n):
    return ceil_div(n, 256) * 256


def dense_mfma_ok(N, c):
    """dense_mfma_ok (lo_dense_mfma.hip)."""
    return c >= 2 and N >= 256


def dense_mfma_tiles(N):
    """dense_mfma_tiles (lo_dense_mfma.hip)."""
    return ceil_div(N, DM_ROWS)


def dense_mfma_slices(B, N, c):
    """dense_mfma_slices (lo_dense_mfma.hip): the slices dense_plan takes partials for."""
    if not dense_mfma_ok(N, c) or c > 20:
        return 1
    wgs = B * dense_mfma_tiles(N)
    ks = min(16, ceil_div(768, wgs))
    ks = min(ks, max(1, N // (4 * DM_KB)))
    return max(1, ks)


def dense_kchunk(B, N, c):
    """(grid.z, kchunk, length of the last slice): the `ks > 1` block of dense_matvec_mfma (lo_dense_mfma.hip)."""
    ks = dense_mfma_slices(B, N, c)
    if ks <= 1:
        return 1, N, N
    kchunk = ceil_div(ceil_div(N, ks), DM_KB) * DM_KB
    gz = ceil_div(N, kchunk)
    return gz, kchunk, N - (gz - 1) * kchunk


def mv16_unal(N, base_misaligned):
    """The `unal` condition of launch_mv16 (lo_dense_mfma.hip), as its causes: "tile" (N % 64 != 0: a ragged last tile),
    "rows" (N % 4 != 0: rows that are not 16-byte aligned) and "base" (the pointer itself)."""
    why = set()
    if N & 63:
        why.add("tile")
    if N & 3:
        why.add("rows")
    if base_misaligned:
        why.add("base")
    return frozenset(why)


def mv16_pad_lds(W, cus):
    """The occupancy branch of launch_mv16 (lo_dense_mfma.hip): 12 KB of unused dynamic LDS for 3 cus < W <= 4 cus."""
    cus = max(64, cus)
    return 3 * cus < W <= 4 * cus


def dense_rows_per_wg(B, N):
    """dense_rows_per_wg (lo_dense.hip)."""
    rows = 128
    while rows > 16 and B * ceil_div(N, rows) < 1024:
        rows //= 2
    return rows


def choose_split(B, N, min_rows=LR_MIN_ROWS, max_split=256):
    """choose_split (lo_vec.hip) -> (S, rows per slice)."""
    S = ceil_div(1024, B)
    maxS = max(1, N // max(min_rows, 4))
    S = max(1, min(S, maxS))
    cap = 64
    while cap < max_split and (cap * 2) * (cap * 2) * 16 <= N:
        cap *= 2
    S = min(S, min(cap, max_split))
    rows = ceil_div(ceil_div(N, S), 4) * 4
    return ceil_div(N, rows), rows


def padded_rank(R):
    """padded_rank (lo_internal.h)."""
    rq, p = ceil_div(R, 4), 1
    while p < rq:
        p <<= 1
    return 4 * p


def skinny_mfma_ok(R4, c):
    """skinny_mfma_ok (lo_skinny_mfma.hip)."""
    return 8 < c <= 32 and R4 in (8, 16, 32, 64, 128)


def lowrank_mv_eligible(R4, N, c):
    """The shape part of lowrank_mv_eligible (lo_lowrank_mv.hip); the rest is the device and LO_NO_RESIDENT_MV."""
    return R4 in (8, 16, 32) and 1 <= c <= 4 and 256 <= N <= 32 * MV_ROWS


def column_chunks(c, width):
    """[(c0, cn)]: the column loop of dense_matvec (width 4), of skinny_tn_impl / skinny_nn (8) and of the c > 20 loop of
    dense_matvec_mfma (32)."""
    return [(c0, min(width, c - c0)) for c0 in range(0, c, width)]


def register_tile(cn):
    """CT of a VALU chunk of cn columns: 1, 2, 4 in dense_matvec; 1, 2, 4, 8 in skinny_tn_impl / skinny_nn."""
    return 1 if cn == 1 else 2 if cn == 2 else 4 if cn <= 4 else 8


def skinny_names(R4, c):
    """The profiler's names of the two passes (tn_name / nn_name of lo_skinny.hip, the scopes of lo_skinny_mfma.hip)."""
    if skinny_mfma_ok(R4, c):
        tail = {32: "_R32", 16: "_R16"}.get(R4, "")
        return "skinny_tn_mfma" + tail, "skinny_nn_mfma" + tail
    return f"skinny_tn_R{R4}", f"skinny_nn_R{R4}"


# ---- the cases -----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Dense:
    group: str            # the route the case is listed for (the parametrised GPU test it runs in)
    B: int
    N: int
    c: int
    diag: str
    misaligned: bool = False   # K is a view one float into a flat buffer: its base is 4 mod 16
    second: str = ""           # non-empty: the case is a further witness of a branch another case reaches, and why it stays

    @property
    def id(self):
        return f"B{self.B}-N{self.N}-c{self.c}-{self.diag}" + ("-base4" if self.misaligned else "")

    @property
    def bound(self):
        return 9 * self.N + 9


@dataclass(frozen=True)
class Lowrank:
    group: str
    B: int
    N: int
    R: int
    c: int
    diag: str
    second: str = ""

    @property
    def id(self):
        return f"B{self.B}-N{self.N}-R{self.R}-c{self.c}-{self.diag}"

    @property
    def bound(self):
        return 27 * self.N * self.R + 9


def _dense_rows(group, rows):
    return tuple(Dense(group, *row[:4], **(row[4] if len(row) > 4 else {})) for row in rows)


BASE4 = {"misaligned": True}

DENSE = (
    # ---- k_dense_mv: below N = 256, and one column at any N
    _dense_rows("valu", (
        (1, 1, 1, "none"), (3, 1, 5, "const"), (1, 3, 2, "full"), (3, 3, 9, "none"), (1, 4, 3, "const"), (3, 4, 4, "full"),
        (1, 5, 5, "full"), (3, 5, 1, "none"), (1, 63, 9, "const"), (3, 63, 2, "none"), (1, 64, 2, "none"),
        (3, 64, 5, "full"), (1, 65, 1, "const"), (3, 65, 3, "full"), (1, 255, 2, "const"), (3, 255, 9, "full"),
        (1, 256, 1, "full"), (1, 257, 1, "none"), (1, 1027, 1, "const"),
        (130, 255, 6, "full"),   # dense_rows_per_wg = 32
        (1, 256, 1, "none", BASE4), (1, 320, 1, "full", BASE4),   # the float4 loads of c = 1 on a base that is 4 mod 16
    ))
    # ---- k_dense_mv_mfma16, one slice
    + _dense_rows("mfma16", (
        (1, 256, 2, "full", {"second": "NV = 0 on aligned rows with B = 1; (1, 1024, 2) reaches it only through the split"}), (3, 256, 17, "none", {"second": "the aligned instantiation with B > 1: members at b N N"}), (1, 257, 15, "const"), (1, 320, 18, "full"), (3, 258, 16, "none"),
        (1, 258, 19, "const"), (1, 319, 20, "full", {"second": "NV = 4 with rows that are not 16-byte aligned, B = 1"}), (3, 319, 2, "none", {"second": "N = 319 with B > 1: the buffer descriptor of a later member starts at an odd float"}), (1, 320, 20, "const"), (1, 320, 19, "none"),
        (1, 321, 17, "full", {"second": "a last tile of one row, B = 1"}), (3, 321, 20, "const", {"second": "a last tile of one row with B > 1 and the constant diagonal per member"}),
        (1, 256, 18, "full", BASE4), (1, 320, 15, "none", BASE4),
    ))
    # ---- k_dense_mv_mfma16 over several slices of K's columns, k_dense_mv_finish
    + _dense_rows("splitk", (
        (1, 1024, 2, "full", {"second": "the issue's B = 1, N = 1024: two equal slices with one member"}),     # two equal slices of 512
        (1, 1100, 17, "none", {"second": "the ragged slice with NV = 1 and one member"}),    # 640 + 460: a ragged slice with a partial last slab
        (1, 1027, 20, "full", {"second": "the N = 1027 the kind is specified at: two slices on rows that are not 16-byte aligned with NV = 4; 2561 and 3585 split such rows too"}),    # 640 + 387, rows that are not 16-byte aligned
        (1, 1536, 17, "full"),    # three equal slices
        (1, 2561, 2, "none"),     # five slices, the last of one column
        (1, 3585, 20, "none"),    # seven slices sized, six launched: the last partial of the workspace stays unwritten
        (3, 1100, 20, "full"),    # members' partials side by side
        (48, 1024, 2, "none"),    # B tiles = 768: the split switches off
        (47, 1024, 2, "full"),    # ... and 752: still two slices
        (52, 1024, 11, "full"),   # 768 < W <= 1024 workgroups: the pad_lds launch on 256 compute units
    ))
    # ---- k_dense_mv_mfma: 21 columns and more, 32 per launch
    + _dense_rows("mfma32", (
        (1, 256, 21, "full", {"second": "21 columns on aligned full tiles: the aligned twin of the base-4 case"}), (3, 256, 32, "none", {"second": "32 live columns on aligned rows with B > 1"}), (1, 257, 31, "const"), (1, 257, 21, "none", {"second": "21 columns on rows that are not 16-byte aligned with B = 1"}), (1, 321, 32, "full"),
        (3, 321, 21, "const", {"second": "a last tile of one row with B > 1 and the constant diagonal"}), (1, 1100, 31, "none"), (1, 1100, 32, "full", {"second": "full and ragged tiles in one launch with all 32 columns live"}),
        (1, 257, 33, "full", {"second": "the 32 | 33 border on rows that are not 16-byte aligned"}), (1, 257, 64, "none"), (1, 320, 52, "const"), (3, 320, 65, "full", {"second": "three column tiles with B > 1"}), (1, 257, 65, "none", {"second": "three column tiles on rows that are not 16-byte aligned"}),
        (1, 320, 33, "none", {"second": "the 32 | 33 border on aligned rows"}),
        (1, 256, 21, "none", BASE4), (1, 320, 32, "full", BASE4),   # the float4 loads of full tiles on a base that is 4 mod 16
    ))
)


def _lowrank_rows(group, rows):
    return tuple(Lowrank(group, *row) for row in rows)


LOWRANK = (
    # ---- the VALU pair k_skinny_tn / k_skinny_nn: c <= 8, c > 32, and every c at R4 = 4 and 256
    _lowrank_rows("valu", (
        # RQ = 1
        (1, 1, 1, 1, "none"), (3, 3, 3, 2, "full"), (1, 255, 4, 3, "const"), (1, 1001, 3, 41, "full"), (3, 257, 4, 9, "none", "the 8 | 9 border at R4 = 4, which the matrix cores do not take: it stays on the VALU pair"),
        (1, 2049, 1, 8, "full", "RQ = 1 over eight slices: 256 row slots, slices of 260 rows leave the 4-rows-in-flight loop idle"),
        # RQ = 2
        (1, 256, 5, 1, "full"), (3, 1001, 8, 2, "none"), (1, 257, 5, 4, "const"), (40, 257, 8, 5, "full", "CT = 8 serving 5 columns as the only chunk, B = 40"),
        (1, 255, 5, 33, "const"),
        # RQ = 4
        (3, 257, 12, 1, "const"), (1, 2049, 16, 2, "full"), (40, 1001, 12, 3, "none"), (1, 1, 16, 8, "full", "one row, eight columns: every slot but one idle in the tn reduction"),
        (3, 256, 12, 41, "full"),
        # RQ = 8
        (40, 256, 17, 1, "none"), (1, 1001, 32, 2, "const"), (3, 2049, 17, 4, "full"), (1, 257, 32, 5, "none", "CT = 8 serving 5 columns without a padded copy"),
        (1, 16385, 17, 33, "full"),   # 64 slices of 260 rows, the last of 5: the shortest last slice min_rows = 256 allows
        # RQ = 16
        (1, 257, 33, 1, "full"), (3, 255, 64, 2, "const"), (1, 1001, 33, 3, "none"), (40, 256, 64, 8, "full", "RQ = 16 with B = 40 and the full diagonal per member"),
        (1, 2049, 33, 41, "const"),
        # RQ = 32
        (3, 1001, 65, 1, "none"), (1, 256, 128, 2, "full"), (1, 3, 65, 4, "full"), (3, 2049, 128, 5, "const", "RQ = 32 over eight slices and three members: the partials of a member are summed, not its neighbour's"),
        (1, 257, 65, 33, "none"),
        # RQ = 64
        (1, 2049, 129, 1, "const"), (3, 257, 256, 2, "none"), (1, 1001, 129, 3, "full"), (1, 255, 256, 8, "full", "RQ = 64, CT = 8: the largest register tile of both kernels"),
        (3, 256, 129, 33, "full", "five chunks at RQ = 64 with B = 3"), (1, 1001, 256, 17, "none", "R4 = 256 at a column count the matrix cores take up to R4 = 128"),
    ))
    # ---- the matrix-core pair k_skinny_tn_mfma / k_skinny_nn_mfma: 8 < c <= 32 at R4 = 8 .. 128
    + _lowrank_rows("mfma", (
        (1, 257, 5, 9, "full"), (3, 1001, 8, 32, "none", "KQ = 1 at 32 columns over three ragged slices, B = 3"), (1, 255, 12, 16, "const"), (40, 257, 16, 17, "full"),
        (1, 2049, 17, 31, "none"), (3, 256, 32, 9, "full"), (1, 1001, 33, 32, "const"), (3, 2049, 64, 17, "full", "NT = 2 over eight slices with B = 3 and the full diagonal"),
        (1, 3, 64, 16, "none"), (1, 257, 65, 16, "full"), (3, 1001, 128, 31, "none", "NT = 4, KQ = 16 at 31 columns: lane 31 of every tile idle"), (1, 2049, 128, 9, "const", "NT = 4 over eight slices: the fixed-order sum of eight partial tiles"),
        (40, 256, 8, 12, "full", "staged tiles of 12 columns with B = 40: 96 float4 per tile, the second trip half idle"),   # c % 4 == 0 and full tiles of 32 rows: the staged v / y tiles of k_skinny_nn_mfma
    ))
)

# the operators of the sum and the mask: one dense and one low-rank term at a ragged N, and a rank the refusal needs
TERM_B, TERM_N, TERM_R = 3, 321, 5
TERM_COLS = (3, 17)
MASK_KEEP = 257        # rows the mask keeps of TERM_N
REFUSED_R = (257, 300)  # padded_rank 512


# ---- route(case) -----------------------------------------------------------------------------------------------------------
def route(case, resident=False, cus=256):
    """{"kernels": {profiler name: launches}, "inst": {template instantiations}, ...}: what serves a case.  `resident`:
    the one-pass low-rank kernel (only where lowrank_mv_eligible).  `cus`: the device's compute units (pad_lds)."""
    if isinstance(case, Dense):
        return _dense_route(case, cus)
    return _lowrank_route(case, resident)


def _dense_route(k, cus):
    B, N, c = k.B, k.N, k.c
    if not dense_mfma_ok(N, c):
        chunks = column_chunks(c, 4)
        branch = "scalar" if N & 3 else "float4"
        rows = dense_rows_per_wg(B, N)
        return {"kernels": {"dense_mv": len(chunks)}, "rows_per_wg": rows, "grid": (ceil_div(N, rows), B), "slices": 1,
                "inst": {("k_dense_mv", register_tile(cn), branch) for _, cn in chunks}, "workspace": 0}
    tiles = dense_mfma_tiles(N)
    if c <= 20:
        gz, kchunk, last = dense_kchunk(B, N, c)
        ks = dense_mfma_slices(B, N, c)
        unal = mv16_unal(N, k.misaligned)
        kernels = {"dense_mv_mfma": 1}
        if gz > 1:
            kernels["dense_mv_finish"] = 1
        return {"kernels": kernels, "inst": {("k_dense_mv_mfma16", max(0, c - 16), bool(unal))}, "unal": unal,
                "slices": gz, "sized_slices": ks, "kchunk": kchunk, "last_slice": last, "grid": (tiles, B, gz),
                "pad_lds": mv16_pad_lds(tiles * B * gz, cus), "workspace": 4 * ks * B * N * c if ks > 1 else 0}
    chunks = column_chunks(c, 32)
    # full_rows of k_dense_mv_mfma per workgroup: N % 4 == 0 and a tile of 64 whole rows
    full = {(N & 3) == 0 and 64 * (t + 1) <= N for t in range(tiles)}
    return {"kernels": {"dense_mv_mfma": len(chunks)}, "slices": 1, "grid": (tiles, B), "workspace": 0,
            "inst": {("k_dense_mv_mfma", len(chunks))} | {("k_dense_mv_mfma", "full_rows", f) for f in full},
            "last_tile_cols": chunks[-1][1]}


def _lowrank_route(k, resident):
    B, N, R, c = k.B, k.N, k.R, k.c
    R4 = padded_rank(R)
    S, rows = choose_split(B, N)
    out = {"R4": R4, "S": S, "rows": rows, "last_rows": N - (S - 1) * rows, "padded_copy": R4 != R,
           "workspace": (align256(4 * B * N * R4) if R4 != R else 0) + 4 * B * S * R4 * c}
    if resident:
        assert lowrank_mv_eligible(R4, N, c)
        return dict(out, kernels={"lr_mv": 1}, inst={("k_lr_mv", R4, register_tile(c))})
    tn, nn = skinny_names(R4, c)
    if skinny_mfma_ok(R4, c):
        return dict(out, kernels={tn: 1, nn: 1}, inst={("k_skinny_tn_mfma", ceil_div(R4, 32)), ("k_skinny_nn_mfma", R4 // 8)})
    chunks = column_chunks(c, 8)
    inst = {(kern, register_tile(cn), R4 // 4) for _, cn in chunks for kern in ("k_skinny_tn", "k_skinny_nn")}
    return dict(out, kernels={tn: len(chunks), nn: len(chunks)}, inst=inst, chunks=chunks)


def term_cases(c):
    """The dense and the low-rank operator of the sum and the mask as cases of their own (no diagonal)."""
    return Dense("term", TERM_B, TERM_N, c, "none"), Lowrank("term", TERM_B, TERM_N, TERM_R, c, "none")


def _merged(*kernel_dicts):
    out = {}
    for d in kernel_dicts:
        for name, n in d.items():
            out[name] = out.get(name, 0) + n
    return out


def sum_kernels(c, resident):
    """{profiler name: launches} of low-rank + dense as LO_OP_SUM: each term's own route (sum_plan gives every term a plan
    of its kind, the resident choice included), and one vec_axpy1 per term behind the first (sum_run, lo_matvec.hip)."""
    dense, lowrank = term_cases(c)
    resident = resident and lowrank_mv_eligible(padded_rank(lowrank.R), lowrank.N, c)
    return _merged(route(lowrank, resident=resident)["kernels"], route(dense)["kernels"], {"vec_axpy1": 1})


def masked_kernels(base, c):
    """{profiler name: launches} of LO_OP_MASKED over the dense ("dense") or low-rank ("lowrank") term
    (masked_matvec_run, lo_masked.hip): the expansion, the base's own route on N0 rows -- a low-rank base keeps to the
    two passes (masked_plan), a dense base that dense_mfma_ok does not take runs k_masked_dense_mv per 4 columns and
    needs no gather -- and the gather."""
    dense, lowrank = term_cases(c)
    if base == "dense" and not dense_mfma_ok(dense.N, c):
        return {"mask_expand": 1, "masked_dense_mv": len(column_chunks(c, 4))}
    inner = route(dense if base == "dense" else lowrank)["kernels"]
    return _merged({"mask_expand": 1}, inner, {"mask_gather": 1})


def split_pattern(k):
    """Which of the row-split patterns of the low-rank table a case is: the slices and its last one."""
    r = _lowrank_route(k, False)
    if k.N < 4:
        return "N<4"
    if r["S"] == 1:
        return "S=1"
    if r["last_rows"] < 8:
        return "S>1,last<8"
    return "S>1,last<rows" if r["last_rows"] < r["rows"] else "S>1,equal"


# ---- inputs and references -------------------------------------------------------------------------------------------------
INTS = np.array([-3, -2, -1, 1, 2, 3], np.float32)


def rng(*key):
    return np.random.Generator(np.random.PCG64([5300, *key]))


def ints(r, shape):
    return INTS[r.integers(0, 6, size=shape, dtype=np.int8)]


def const_diag(B):
    """One of 1, 2, 3 per member, neighbours different: what LO_DIAG_CONST reads at dd[b]."""
    return (np.arange(B) % 3 + 1).astype(np.float32)


def full_diag(r, B, N):
    return r.integers(1, 4, size=(B, N)).astype(np.float32)


def diag_term(d, v, mode):
    """d o v in int64 for mode "none" / "full" (d [B, N]) / "const" (d [B])."""
    if mode == "none":
        return 0
    d = d.astype(np.int64)
    return (d[:, :, None] if mode == "full" else d[:, None, None]) * v.astype(np.int64)


def diag_of(data, mode):
    return {"none": None, "full": data["d_full"], "const": data["d_const"]}[mode]


def _frozen(data):
    for a in data.values():
        a.setflags(write=False)
    return data


def dense_product(K, v):
    """K v in int64, a member at a time."""
    return np.stack([K[b].astype(np.int64) @ v[b].astype(np.int64) for b in range(K.shape[0])])


def lowrank_product(C, v):
    """C (C^T v) in int64."""
    C64, v64 = C.astype(np.int64), v.astype(np.int64)
    return np.matmul(C64, np.matmul(C64.transpose(0, 2, 1), v64))


@functools.lru_cache(maxsize=4)
def dense_data(B, N, c):
    """{K [B, N, N], v [B, N, c], d_full [B, N], d_const [B], Kv (int64)} of a dense shape; members differ."""
    r = rng(1, B, N, c)
    K, v = ints(r, (B, N, N)), ints(r, (B, N, c))
    return _frozen({"K": K, "v": v, "d_full": full_diag(r, B, N), "d_const": const_diag(B), "Kv": dense_product(K, v)})


@functools.lru_cache(maxsize=8)
def lowrank_data(B, N, R, c):
    """{C [B, N, R], v [B, N, c], d_full, d_const, CCv (int64)} of a low-rank shape."""
    r = rng(2, B, N, R, c)
    C, v = ints(r, (B, N, R)), ints(r, (B, N, c))
    return _frozen({"C": C, "v": v, "d_full": full_diag(r, B, N), "d_const": const_diag(B), "CCv": lowrank_product(C, v)})


def reference(case):
    """The int64 product of a case with its diagonal."""
    if isinstance(case, Dense):
        data = dense_data(case.B, case.N, case.c)
        return data["Kv"] + diag_term(diag_of(data, case.diag), data["v"], case.diag)
    data = lowrank_data(case.B, case.N, case.R, case.c)
    return data["CCv"] + diag_term(diag_of(data, case.diag), data["v"], case.diag)


def mask_rows(N0, keep):
    """`keep` strictly increasing rows of N0, the first and the last among them."""
    inner = np.sort(rng(3, N0, keep).permutation(N0 - 2)[:keep - 2]) + 1
    return np.concatenate(([0], inner, [N0 - 1])).astype(np.int64)


# ---- the checker -----------------------------------------------------------------------------------------------------------
def exact(got, ref):
    """Whether the float32 array `got` IS the int64 array `ref`: equal element for element after casting ref to float32,
    which must lose nothing."""
    ref = np.asarray(ref)
    assert ref.dtype == np.int64, ref.dtype
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32.astype(np.int64), ref), "the reference is not representable in float32"
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
