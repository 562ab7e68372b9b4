"""The edge cases of the dense and low-rank matvecs without a GPU (tests/dense_lowrank_edge_cases.py): the restated launch
arithmetic gives the splits the shapes were chosen for and the workspace sizes the library reports, every template
instantiation and dispatch border the tables are listed for is reached by a row, every row keeps float32 sums exact, the
int64 references are what float64 gives, and no row is idle: the coverage checks are functions of a table, and they are
run again on the table without each row in turn -- a row whose removal they do not notice must say whose second witness
it is.  These are conditions on the inputs of tests/test_gpu_dense_lowrank_edges.py."""
import ctypes

import numpy as np
import pytest
import torch

import dense_lowrank_edge_cases as E
from linear_operator_amd import _hip
from linear_operator_amd.kernels import OperatorDescriptor

ISSUE_DENSE_VALU_N, ISSUE_DENSE_VALU_C = {1, 3, 4, 5, 63, 64, 65, 255}, {1, 2, 3, 4, 5, 9}
ISSUE_MFMA16_N, ISSUE_MFMA16_C = {256, 257, 258, 319, 320, 321}, {2, 15, 16, 17, 18, 19, 20}
ISSUE_RANKS = {1, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 65, 128, 129, 256}
ISSUE_LOWRANK_C = {1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 41}
ISSUE_LOWRANK_N, ISSUE_LOWRANK_B = {1, 3, 255, 256, 257, 1001, 2049}, {1, 3, 40}


def group(table, name):
    return [k for k in table if k.group == name]


# ---- the restated arithmetic ---------------------------------------------------------------------------------------------
def test_dense_splits_are_the_ones_the_shapes_were_chosen_for():
    want = {(1, 1024, 2): (2, 512, 512), (1, 1100, 17): (2, 640, 460), (1, 1027, 20): (2, 640, 387),
            (1, 1536, 17): (3, 512, 512), (1, 2561, 2): (5, 640, 1), (1, 3585, 20): (6, 640, 385),
            (3, 1100, 20): (2, 640, 460), (48, 1024, 2): (1, 1024, 1024), (47, 1024, 2): (2, 512, 512),
            (52, 1024, 11): (1, 1024, 1024)}
    assert set(want) == {(k.B, k.N, k.c) for k in group(E.DENSE, "splitk")}
    for shape, split in want.items():
        assert E.dense_kchunk(*shape) == split, shape
        assert split[1] % E.DM_KB == 0 or split[0] == 1
    assert E.dense_mfma_slices(1, 3585, 20) == 7          # sized for seven, six launched
    assert E.dense_mfma_slices(1, 1024, 21) == 1          # the 32-wide kernel never splits
    assert E.dense_mfma_slices(1, 1023, 2) == 1           # fewer than four slabs per slice
    assert E.dense_mfma_slices(1, 16384, 17) == 3 and E.dense_mfma_slices(1, 100000, 2) == 1
    assert 48 * E.dense_mfma_tiles(1024) == 768 and 52 * E.dense_mfma_tiles(1024) == 832
    assert E.mv16_pad_lds(832, 256) and not E.mv16_pad_lds(768, 256) and E.mv16_pad_lds(1024, 256)
    assert not E.mv16_pad_lds(1025, 256) and not E.mv16_pad_lds(832, 304)
    assert E.dense_rows_per_wg(130, 255) == 32 and E.dense_rows_per_wg(1, 255) == 16 and E.dense_rows_per_wg(1, 10 ** 6) == 128
    assert not E.dense_mfma_ok(255, 9) and not E.dense_mfma_ok(4096, 1) and E.dense_mfma_ok(256, 2)
    assert E.mv16_unal(256, False) == set() and E.mv16_unal(256, True) == {"base"} and E.mv16_unal(258, False) == {"tile", "rows"}
    assert E.mv16_unal(260, False) == {"tile"}


def test_lowrank_splits_ranks_and_borders():
    assert [E.padded_rank(R) for R in sorted(ISSUE_RANKS)] == [4, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256]
    assert E.padded_rank(257) == 512 and all(E.padded_rank(R) > E.MAX_RANK for R in E.REFUSED_R)
    assert E.choose_split(1, 1001) == (3, 336) and E.choose_split(1, 2049) == (8, 260) and E.choose_split(40, 2049) == (8, 260)
    assert E.choose_split(1, 257) == (1, 260) and E.choose_split(1, 3) == (1, 4) and E.choose_split(1, 16385) == (64, 260)
    assert E.choose_split(512, 8192) == (2, 4096) and E.choose_split(1, 1 << 20) == (256, 4096)
    assert not E.skinny_mfma_ok(32, 8) and E.skinny_mfma_ok(32, 9) and E.skinny_mfma_ok(32, 32) and not E.skinny_mfma_ok(32, 33)
    assert not E.skinny_mfma_ok(4, 16) and not E.skinny_mfma_ok(256, 16)
    assert E.column_chunks(33, 8) == [(0, 8), (8, 8), (16, 8), (24, 8), (32, 1)] and E.column_chunks(52, 32) == [(0, 32), (32, 20)]
    assert E.column_chunks(9, 4) == [(0, 4), (4, 4), (8, 1)]
    assert E.lowrank_mv_eligible(8, 256, 4) and not E.lowrank_mv_eligible(8, 255, 4) and not E.lowrank_mv_eligible(64, 256, 1)
    assert not E.lowrank_mv_eligible(8, 256, 5) and E.lowrank_mv_eligible(32, 32768, 1) and not E.lowrank_mv_eligible(32, 32769, 1)


def split_all(S0, N):
    """choose_split for one first guess S0 = ceil(1024 / B) and an int64 array of N, step by step as lo_vec.hip has it."""
    S = np.maximum(1, np.minimum(S0, np.maximum(1, N // max(E.LR_MIN_ROWS, 4))))
    cap = np.full_like(N, 64)
    for _ in range(2):   # the doubling loop of the slice cap: 64 -> 128 -> 256
        cap = np.where((cap < 256) & ((cap * 2) * (cap * 2) * 16 <= N), cap * 2, cap)
    S = np.minimum(S, cap)
    rows = (-(-N // S) + 3) // 4 * 4
    return -(-N // rows), rows


def test_what_the_row_split_cannot_reach():
    """The issue lists a last row slice of fewer than 4 rows with S > 1, and NT = 3.  Neither exists: with min_rows = 256
    the shortest last slice of a split member is 5 rows, at N = 16385; and padded ranks are 4 times a power of two, so
    ceil(R4 / 32) is 1, 2 or 4 (8 is refused by the MFMA gate).  The table holds N = 16385, and N < 4 for slices shorter
    than a quad.  The search runs on a vector form of choose_split, which is compared with E.choose_split itself on
    every N below 6000, on a stride through the rest, at the borders of the slice cap and around every minimum."""
    N = np.arange(1, 621001, dtype=np.int64)   # every N a rank >= 1 can have within the bound
    sample = np.unique(np.concatenate((np.arange(1, 6000), np.arange(6000, 621001, 613),
                                       [16383, 16384, 16385, 262143, 262144, 262145, 621000])))
    shortest = {}
    for S0 in sorted({E.ceil_div(1024, B) for B in range(1, 1100)}):
        S, rows = split_all(S0, N)
        last = np.where(S > 1, N - (S - 1) * rows, 1 << 40)
        i = int(np.argmin(last))
        shortest[S0] = (int(last[i]), int(N[i]))
        B = E.ceil_div(1024, S0)
        assert E.ceil_div(1024, B) == S0
        for n in np.concatenate((sample, np.arange(max(1, N[i] - 8), min(621000, N[i] + 8) + 1))):
            assert E.choose_split(B, int(n)) == (int(S[n - 1]), int(rows[n - 1])), (B, n)
    assert min(shortest.values()) == (5, 16385)
    assert {E.ceil_div(E.padded_rank(R), 32) for R in range(1, 257) if E.skinny_mfma_ok(E.padded_rank(R), 16)} == {1, 2, 4}


def desc_of(k):
    """A descriptor over CPU tensors that are never read: the sizers look at the shape alone."""
    any_ = torch.zeros(4)
    if isinstance(k, E.Dense):
        d = OperatorDescriptor(_hip.LO_OP_DENSE_DIAG, k.B, k.N, A0=any_)
    else:
        d = OperatorDescriptor(_hip.LO_OP_LOWRANK_DIAG, k.B, k.N, A0=any_, R=k.R)
    if k.diag != "none":
        d.d, d.diag_mode = any_, (_hip.LO_DIAG_CONST if k.diag == "const" else _hip.LO_DIAG_FULL)
    return d


@pytest.mark.parametrize("k", E.DENSE + E.LOWRANK, ids=lambda k: f"{type(k).__name__}-{k.group}-{k.id}")
def test_the_reported_workspace_holds_what_the_route_takes(k):
    """lo_matvec_workspace_bytes >= 256 + the split-K partials, or the padded copy of C and tpart; in fact equal."""
    s = desc_of(k).c_struct()
    got = int(_hip.load().lo_matvec_workspace_bytes(ctypes.byref(s), k.c))
    need = E.route(k)["workspace"]
    assert got >= E.PLAN_TAIL + need
    assert got == E.PLAN_TAIL + need, (got, need)


def test_a_refused_rank_is_sized_without_its_buffers():
    for R in E.REFUSED_R:
        s = desc_of(E.Lowrank("refused", 2, 300, R, 3, "full")).c_struct()
        assert int(_hip.load().lo_matvec_workspace_bytes(ctypes.byref(s), 3)) <= E.PLAN_TAIL


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def test_every_case_keeps_float32_sums_exact():
    worst = max(k.bound for k in E.DENSE + E.LOWRANK)
    print(f"largest bound: {worst} of {E.LIMIT}")
    assert worst < E.LIMIT
    assert all(k.N * k.R <= 621000 for k in E.LOWRANK)
    # the sum and the mask: a low-rank term, a dense term and one diagonal
    assert 27 * E.TERM_N * E.TERM_R + 9 * E.TERM_N + 9 < E.LIMIT


def small(k):
    return k.B * k.N * (k.N if isinstance(k, E.Dense) else k.R) <= 1 << 22


@pytest.mark.parametrize("k", [k for k in E.DENSE + E.LOWRANK if small(k) or k.N == 3585],
                         ids=lambda k: f"{type(k).__name__}-{k.group}-{k.id}")
def test_the_int64_reference_is_the_float64_product(k):
    """... of the same inputs, and stays within the case's bound: float32 holds it."""
    if isinstance(k, E.Dense):
        data = E.dense_data(k.B, k.N, k.c)
        f64 = data["K"].astype(np.float64) @ data["v"].astype(np.float64)
        ints_of = (data["K"], data["v"])
    else:
        data = E.lowrank_data(k.B, k.N, k.R, k.c)
        C64 = data["C"].astype(np.float64)
        f64 = C64 @ (C64.transpose(0, 2, 1) @ data["v"].astype(np.float64))
        ints_of = (data["C"], data["v"])
    for a in ints_of:
        assert set(np.unique(a).tolist()) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert set(np.unique(data["d_full"]).tolist()) <= {1.0, 2.0, 3.0} and set(np.unique(data["d_const"]).tolist()) <= {1.0, 2.0, 3.0}
    d = E.diag_of(data, k.diag)
    f64 = f64 + (0.0 if d is None else (d[:, :, None] if k.diag == "full" else d[:, None, None]).astype(np.float64) * data["v"])
    ref = E.reference(k)
    assert ref.dtype == np.int64 and np.array_equal(ref.astype(np.float64), f64)
    assert np.abs(ref).max() <= k.bound
    assert E.exact(ref.astype(np.float32), ref)
    if k.B > 1:   # members differ, and so do their constant diagonals
        assert not np.array_equal(ints_of[0][0], ints_of[0][1]) and data["d_const"][0] != data["d_const"][1]


def test_the_checker_takes_nothing_but_the_reference():
    ref = np.array([[1, -25], [16777215, 3]], np.int64)
    assert E.exact(ref.astype(np.float32), ref)
    assert not E.exact(np.nextafter(ref.astype(np.float32), np.float32(9)), ref)
    assert not E.exact(ref.astype(np.float32).ravel(), ref)
    bad = ref.astype(np.float32)
    bad[0, 1] = np.nan
    assert not E.exact(bad, ref) and "(0, 1)" in E.mismatches(bad, ref)
    with pytest.raises(AssertionError):
        E.exact(ref.astype(np.float32), ref + (1 << 24))    # 2^24 + 1: a reference float32 cannot hold
    with pytest.raises(AssertionError):
        E.exact(ref.astype(np.float64), ref)                # float64 is not what a kernel returns


def test_one_wrong_term_at_an_edge_is_seen():
    """What three mistakes the kernels' guards exist against do to a result.  A slab of K's columns counted by neither
    slice, or by a chunk's partials read at another chunk's offset, moves the product, since every entry is non-zero.  A
    load guard that lets column N of a row through (`gk + e <= N`) does NOT move it as long as what it reads is finite:
    the element meets the v slab's entry for k = N, which that slab's own guard has zeroed.  Only a NaN behind the last
    row of the last member shows it, as 0 * NaN in that row -- which is why the GPU test keeps K between NaN bands."""
    data = E.dense_data(1, 257, 21)
    K, v, ref = data["K"][0].astype(np.float64), data["v"][0].astype(np.float64), data["Kv"]
    N = K.shape[0]
    flat = np.concatenate((K.ravel(), [np.nan]))                 # K and the first float of the band behind it
    over = flat[np.arange(1, N + 1) * N]                         # what row i reads at column N: K[i + 1][0], then the band
    with np.errstate(invalid="ignore"):
        got = K @ v + over[:, None] * np.zeros_like(v[:1])       # ... times the zeroed entry of the v slab
    assert np.array_equal(got[:-1], ref[0, :-1].astype(np.float64)) and np.isnan(got[-1]).all()
    assert not E.exact(got[None].astype(np.float32), ref)
    data = E.dense_data(1, 1100, 17)
    _, kchunk, _ = E.dense_kchunk(1, 1100, 17)
    cut = data["K"].copy()
    cut[0, :, 550:kchunk] = 0            # kchunk = 550: the slab that straddles the slices is read by neither
    assert not E.exact(E.dense_product(cut, data["v"]).astype(np.float32), data["Kv"])
    data = E.lowrank_data(1, 1001, 3, 41)
    C, v = data["C"], data["v"]
    wrong = v.copy()
    wrong[..., 8:16] = v[..., 0:8]        # the c0 offset of tpart dropped: chunk 1 reads chunk 0's t
    got = E.lowrank_product(C, v)
    got[..., 8:16] = E.lowrank_product(C, wrong)[..., 8:16]
    assert not E.exact(got.astype(np.float32), data["CCv"])


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def features(k):
    """The things a case is a witness of; each kind of entry is asserted by check_dense / check_lowrank below."""
    r = E.route(k)
    f = {("inst",) + tuple(i) for i in r["inst"]}
    if isinstance(k, E.Dense):
        if k.group == "valu":
            f |= {("rows_per_wg", r["rows_per_wg"]), ("valu passes", r["kernels"]["dense_mv"]), ("valu N<4", k.N < 4)}
        if "unal" in r:
            tiles = k.B * E.dense_mfma_tiles(k.N)
            f |= {("unal", tuple(sorted(r["unal"]))), ("slices", min(r["slices"], 3), r["last_slice"] < r["kchunk"]),
                  ("last slab", r["last_slice"] % E.DM_KB != 0, r["slices"] > 1), ("pad_lds", r["pad_lds"]),
                  ("sized > launched", r["sized_slices"] > r["slices"]), ("split, unal", r["slices"] > 1, bool(r["unal"])),
                  ("split, B>1", r["slices"] > 1, k.B > 1), ("split, last slice of", min(r["last_slice"], 2)),
                  ("ragged slice, B>1", r["slices"] > 1 and r["last_slice"] < r["kchunk"] and k.B > 1)}
            if tiles in (752, 768):   # either side of the batch at which the split switches off
                f.add(("B tiles", tiles))
        if k.c > 20:
            f |= {("column tiles", r["kernels"]["dense_mv_mfma"], "last of", r["last_tile_cols"]),
                  ("mfma32 c, rows 16-byte aligned", min(k.c, 33), k.N % 4 == 0)}
        return f
    f |= {("split", E.split_pattern(k)), ("split", k.group, E.split_pattern(k)), ("padded copy", k.group, r["R4"], r["padded_copy"]),
          ("R4 on", k.group, r["R4"])}
    if E.lowrank_mv_eligible(r["R4"], k.N, k.c):
        f.add(("resident twin", r["R4"], E.register_tile(k.c)))
    if k.group == "valu":   # a chunk behind the first reads v, y and tpart at its column offset
        f |= {("chunk", "first" if c0 == 0 else "later", E.register_tile(cn), r["R4"] // 4) for c0, cn in r["chunks"]}
    if k.group == "mfma":
        f.add(("staged tiles", k.c % 4 == 0 and r["rows"] >= 32 and k.N >= 128))
    return f


def all_features(table):
    out = set()
    for k in table:
        out |= features(k)
    return out


def check_dense(table):
    """Every branch the dense table is listed for is reached by a row of `table`."""
    f = all_features(table)
    valu, m16, sk, m32 = (group(table, g) for g in ("valu", "mfma16", "splitk", "mfma32"))
    # k_dense_mv<1 | 2 | 4> in both N & 3 branches; several 4-column passes; N < 4; rows_per_wg above 16
    assert {("inst", "k_dense_mv", ct, br) for ct in (1, 2, 4) for br in ("float4", "scalar")} <= f
    assert {("valu passes", 2), ("valu passes", 3), ("valu N<4", True), ("rows_per_wg", 32), ("rows_per_wg", 16)} <= f
    assert ISSUE_DENSE_VALU_N <= {k.N for k in valu} and ISSUE_DENSE_VALU_C <= {k.c for k in valu if k.N < 256}
    assert {(k.N, k.c) for k in valu if k.N >= 256 and not k.misaligned} == {(256, 1), (257, 1), (1027, 1)}
    for n in ISSUE_DENSE_VALU_N:
        assert {k.B for k in valu if k.N == n} >= {1, 3}, n
    # k_dense_mv_mfma16<NV = 0 .. 4, UNAL = false | true>, UNAL by the tile, by the rows and by the base alone
    assert {("inst", "k_dense_mv_mfma16", nv, u) for nv in range(5) for u in (False, True)} <= f
    assert {("unal", ("base",)), ("unal", ("tile",)), ("unal", ("rows", "tile")), ("unal", ())} <= f
    assert {k.N for k in m16} == ISSUE_MFMA16_N and {k.c for k in m16} == ISSUE_MFMA16_C
    # slices 1, 2 and >= 3 with a ragged last one; the split with unaligned rows, with members, sized beyond launched,
    # switched off by the batch (and not yet, one member before), and the occupancy branch
    assert {("slices", 1, False), ("slices", 2, False), ("slices", 2, True), ("slices", 3, False), ("slices", 3, True)} <= f
    assert {("split, unal", True, True), ("split, unal", True, False), ("split, B>1", True, True), ("sized > launched", True),
            ("pad_lds", True), ("last slab", True, True), ("split, last slice of", 1), ("ragged slice, B>1", True),
            ("B tiles", 752), ("B tiles", 768)} <= f
    assert {k.c for k in sk} >= {2, 17, 20} and {k.diag for k in sk} == {"full", "none"}
    assert any("rows" in E.route(k)["unal"] and E.route(k)["slices"] > 1 for k in sk)
    # k_dense_mv_mfma with one, two and three column tiles, both full_rows outcomes; c = 21, 31, 32 and a later tile, each
    # on rows that are 16-byte aligned and on rows that are not
    assert {("inst", "k_dense_mv_mfma", n) for n in (1, 2, 3)} <= f
    assert {("inst", "k_dense_mv_mfma", "full_rows", True), ("inst", "k_dense_mv_mfma", "full_rows", False)} <= f
    assert {("mfma32 c, rows 16-byte aligned", c, a) for c in (21, 31, 32, 33) for a in (True, False)} <= f
    assert {k.N for k in m32 if k.c <= 32} >= {256, 257, 321, 1100} and {k.c for k in m32} == {21, 31, 32, 33, 52, 64, 65}
    assert {k.N for k in m32 if k.c > 32} == {257, 320}
    assert {("column tiles", 2, "last of", 1), ("column tiles", 2, "last of", 20), ("column tiles", 3, "last of", 1),
            ("column tiles", 2, "last of", 32)} <= f
    for g in ("valu", "mfma16", "mfma32"):
        assert {k.diag for k in group(table, g)} == set(E.DIAG_MODES), g
    # a base that is 4 mod 16 at N = 256 and 320 on each route: under the 16-wide kernel, which looks at the pointer, and
    # under the float4 loads that do not (c = 1 and c >= 21 at N % 4 == 0)
    for g in ("valu", "mfma16", "mfma32"):
        assert {k.N for k in group(table, g) if k.misaligned} == {256, 320}, g
    assert {k.c for k in valu if k.misaligned} == {1} and 21 in {k.c for k in m32 if k.misaligned}


def check_lowrank(table):
    """Every branch the low-rank table is listed for is reached by a row of `table`."""
    f = all_features(table)
    cts, rqs = (1, 2, 4, 8), (1, 2, 4, 8, 16, 32, 64)
    assert {("inst", kern, ct, rq) for kern in ("k_skinny_tn", "k_skinny_nn") for ct in cts for rq in rqs} <= f
    assert {("inst", "k_skinny_tn_mfma", nt) for nt in (1, 2, 4)} <= f        # (NT = 3: test_what_the_row_split_cannot_reach)
    assert {("inst", "k_skinny_nn_mfma", kq) for kq in (1, 2, 4, 8, 16)} <= f
    assert {k.R for k in table} == ISSUE_RANKS and {k.c for k in table} >= ISSUE_LOWRANK_C
    assert {k.N for k in table} >= ISSUE_LOWRANK_N and {k.B for k in table} == ISSUE_LOWRANK_B
    assert {("R4 on", "valu", r4) for r4 in (4, 8, 16, 32, 64, 128, 256)} <= f
    assert {("R4 on", "mfma", r4) for r4 in (8, 16, 32, 64, 128)} <= f
    assert {("split", p) for p in ("S=1", "S>1,last<rows", "S>1,last<8", "N<4")} <= f
    assert {("split", "mfma", p) for p in ("S=1", "S>1,last<rows", "N<4")} <= f
    # the column borders 8 | 9 and 32 | 33 at a rank the matrix cores take, every chunk remainder, and at every width a
    # chunk behind the first, of eight columns and of one (v, y and tpart read at the chunk's offset)
    for c in (8, 9, 32, 33):
        assert any(k.c == c and E.route(k)["R4"] in (8, 16, 32, 64, 128) for k in table), c
    assert {cn for k in group(table, "valu") for _, cn in E.route(k)["chunks"]} == {1, 2, 3, 4, 5, 8}
    assert {("chunk", "later", ct, rq) for ct in (1, 8) for rq in rqs} <= f
    assert {("chunk", "first", ct, rq) for ct in cts for rq in rqs} <= f
    # pad_rows at every width, and no copy at every width; before the matrix-core pair too
    assert {("padded copy", "valu", r4, p) for r4 in (4, 8, 16, 32, 64, 128, 256) for p in (True, False)} <= f
    assert {("padded copy", "mfma", r4, p) for r4 in (8, 16, 32, 64, 128) for p in (True, False)} <= f
    assert {("staged tiles", True), ("staged tiles", False)} <= f
    assert {("resident twin", r4, ct) for r4 in (8, 16, 32) for ct in (1, 2, 4)} <= f
    for g in ("valu", "mfma"):
        assert {k.diag for k in group(table, g)} == set(E.DIAG_MODES), g


def test_the_dense_table_reaches_every_branch():
    check_dense(E.DENSE)


def test_the_lowrank_table_reaches_every_branch():
    check_lowrank(E.LOWRANK)


def unnoticed(table, check):
    """The rows of `table` whose removal `check` does not notice."""
    out = []
    for i, k in enumerate(table):
        try:
            check(table[:i] + table[i + 1:])
        except AssertionError:
            continue
        out.append(k)
    return out


@pytest.mark.parametrize("table,check", ((E.DENSE, check_dense), (E.LOWRANK, check_lowrank)), ids=("dense", "lowrank"))
def test_no_case_is_idle(table, check):
    """Taking any one case out of a table fails the coverage check of that table, or the case says whose second witness it
    is; and a case that says so is one the check can indeed do without."""
    assert len({(k.group, k.id) for k in table}) == len(table)
    idle = unnoticed(table, check)
    for k in table:
        if k.second:
            print(f"{k.group} {k.id}: second witness -- {k.second}")
    assert [k.id for k in idle if not k.second] == []
    assert [k.id for k in table if k.second and k not in idle] == []
