"""The edge cases of the Kronecker matvecs without a GPU (tests/kron_edge_cases.py): every engine, template
instantiation and named edge the tables are listed for is reached by a row of `route()`, every row keeps float32 sums
exact and its footprint under the cap, no factor is symmetric, the float64 references are what an int64 einsum gives,
a transposed factor moves every reference, and the restated workspace sizes and dot-partial counts are the ones the host
library reports.  These are conditions on the inputs of tests/test_gpu_kron_edges.py."""
import ctypes

import numpy as np
import pytest
import torch

import kron_edge_cases as E
from linear_operator_amd import _hip
from linear_operator_amd import kernels as K
from linear_operator_amd.kernels import OperatorDescriptor

SMALL = 4096   # n1 n2 up to which the int64 einsum is run


def ids(k):
    return f"{k.group}-{k.id}"


def edges(table, **kw):
    out = set()
    for k in table:
        out |= E.route(k, **kw)["edges"]
    return out


def insts(table, **kw):
    out = set()
    for k in table:
        out |= E.route(k, **kw)["inst"]
    return out


# ---- the restated arithmetic ---------------------------------------------------------------------------------------------
def test_the_gates_and_grids_are_the_ones_the_shapes_were_chosen_for():
    assert E.kron_mfma_ok(64, 64, 1) and not E.kron_mfma_ok(64, 64, 2) and not E.kron_mfma_ok(60, 64, 1)
    assert not E.kron_mfma_ok(65, 68, 1) and not E.kron_mfma_ok(64, 66, 1) and E.kron_mfma_ok(68, 132, 1)
    assert E.kron_mfma_cols_ok(64, 64, 2) and E.kron_mfma_cols_ok(64, 64, 64) and not E.kron_mfma_cols_ok(64, 64, 65)
    assert not E.kron_mfma_cols_ok(64, 64, 1) and not E.kron_mfma_cols_ok(64, 66, 2)
    assert E.kron_fused_ok(128, 384) and E.kron_fused_ok(256, 128) and not E.kron_fused_ok(384, 128)
    assert not E.kron_fused_ok(128, 192) and not E.kron_fused_ok(128, 128, no_fused=True)
    assert E.kron_fused_taken(96, 128, 128) and not E.kron_fused_taken(95, 128, 128) and E.kron_fused_taken(48, 256, 256)
    assert not E.kron_fused_taken(47, 128, 256) and E.kron_fused_taken(32, 128, 384) and not E.kron_fused_taken(31, 256, 384)
    assert [E.fused_inst(*s) for s in ((128, 128), (128, 256), (128, 384), (256, 256), (256, 128), (256, 384))] == \
        [(4, 2), (4, 0), (4, 0), (8, 4), (8, 0), (8, 0)]
    assert E.km_aligned(128, 384) and not E.km_aligned(128, 68) and not E.km_aligned(64, 64)
    assert E.kron_S_dot(260, 132, 1, 5) == 6 and E.kron_S_dot(384, 384, 1, 5) == 9 and E.kron_S_dot(64, 64, 1, 5) == 1
    assert E.kron_S_dot(260, 132, 3, 5) == 5 and E.kron_S_dot(65, 68, 1, 7) == 7
    assert E.gemm_grid(65, 65, 3) == (2, 2, 3) and E.gemm_grid(64, 64 * 65, 1) == (65, 1, 1) and E.gemm_grid(1, 1, 17) == (1, 1, 17)
    assert E.km_grid(132, 260, 9) == 16 * 6 and E.km_grid(128, 128, 8) == 8 and E.km_grid(64, 64, 1) == 8
    assert E.km_grid(68, 68, 51) == 56 and E.fused_grid(97, 128) == 104 and E.fused_grid(49, 256) == 112
    assert E.cols_grid(3, 4624) == (19, 3) and 4624 - 18 * 256 == 16 and E.cols_grid(1, 4352) == (17, 1)
    assert E.cols_lds_bytes(64) == 66560 and E.cols_lds_bytes(63) == 64512 and E.cols_lds_bytes(2) == 3072
    assert E.kron_workspace_floats(3, 64, 68, 3) == 2 * 3 * 4352 * 3 and E.kron_workspace_floats(3, 64, 68, 1) == 3 * 4352
    assert E.kron_workspace_floats(1, 64, 64, 65) == 4096 * 65
    assert E.f64_grids(3, 16, 33, 2) == {"pass1": (1, 2, 3), "pass2": (3, 1, 3), "kfast": True}
    assert E.f64_grids(1, 33, 33, 9)["pass1"] == (10, 2, 1) and not E.f64_grids(1, 32, 32, 8)["kfast"] and E.f64_grids(1, 32, 16, 7)["kfast"]
    assert E.choose_split(1, 1001) == (3, 336) and E.choose_split(1024, 147456) == (1, 147456)


def desc_of(k):
    """A descriptor over CPU tensors that are never read: the sizers look at the shape alone."""
    any_ = torch.zeros(4, dtype=torch.float64 if k.f64 else torch.float32)
    d = OperatorDescriptor(_hip.LO_OP_KRON_DIAG, k.B, k.N, A0=any_, A1=any_, R=k.n1, n2=k.n2, dtype=any_.dtype)
    if k.diag != "none":
        d.d, d.diag_mode = any_, (_hip.LO_DIAG_CONST if k.diag == "const" else _hip.LO_DIAG_FULL)
    return d


@pytest.mark.parametrize("k", E.ALL + E.MISALIGNED + (E.REFUSED,), ids=ids)
def test_the_reported_workspace_is_the_restated_one(k):
    """lo_matvec_workspace_bytes = 256 + one buffer of B N c floats, two on the many-column route; the float64 sizer
    1024 + one buffer of doubles."""
    s = desc_of(k).c_struct(torch.float64 if k.f64 else torch.float32)
    sizer = _hip.load().lo_matvec_f64_workspace_bytes if k.f64 else _hip.load().lo_matvec_workspace_bytes
    assert int(sizer(ctypes.byref(s), k.c)) == k.workspace_bytes
    assert E.route(k)["workspace"] == k.itemsize * k.B * k.N * k.c * (2 if E.route(k)["engine"] == "cols" else 1)


def cg_bytes(n1, n2, B, c):
    s = desc_of(E.Kron("sizer", n1, n2, c, B, "none")).c_struct()
    prm = K._cg_params(c, 0, 1, 1, 1e-6, 1e-10, 1e-10, 0)
    return int(_hip.load().lo_cg_workspace_bytes(ctypes.byref(s), None, ctypes.byref(prm)))


SHAPES = sorted({(k.n1, k.n2) for k in E.ALL if not k.f64} | {s[:2] for s in E.CG_STEP})


@pytest.mark.parametrize("n1,n2", SHAPES, ids=lambda n: str(n))
def test_the_restated_dot_partial_count_is_the_one_the_cg_workspace_is_sized_for(n1, n2):
    """kron_S_dot has no entry point of its own; lo_cg_workspace_bytes takes B max(S_dot, S) c floats for the partials
    (cg_layout, lo_cg.hip).  At B = 1024 the row split is S = 1, and N (x) 1 is the same operator size on the VALU
    route (S_dot = S): the two workspaces differ by 4 B (S_dot - 1) bytes.  With three columns no route fuses the
    partials, and the sizes differ by the second buffer of the many-column route alone."""
    B = 1024
    assert E.choose_split(B, n1 * n2)[0] == 1
    want = E.kron_S_dot(n1, n2, 1, 1)
    assert want == (E.km_tiles(n1, n2) if E.kron_mfma_ok(n1, n2, 1) else 1)
    assert cg_bytes(n1, n2, B, 1) - cg_bytes(n1 * n2, 1, B, 1) == 4 * B * (want - 1)
    second = 4 * (E.kron_workspace_floats(B, n1, n2, 3) - B * n1 * n2 * 3)
    assert second == (4 * B * n1 * n2 * 3 if E.kron_mfma_cols_ok(n1, n2, 3) else 0)
    assert E.kron_S_dot(n1, n2, 3, 1) == 1 and cg_bytes(n1, n2, B, 3) - cg_bytes(n1 * n2, 1, B, 3) == second


# ---- the inputs ------------------------------------------------------------------------------------------------------------
def test_every_case_keeps_float32_sums_exact_and_its_footprint_under_the_cap():
    every = E.ALL + E.MISALIGNED
    worst = max(every, key=lambda k: k.bound)
    print(f"largest bound: {worst.bound} of {E.LIMIT} at {ids(worst)}")
    assert all(k.bound < E.LIMIT for k in every)
    big = max(every, key=lambda k: k.footprint)
    print(f"largest footprint: {big.footprint / 2 ** 20:.1f} MiB at {ids(big)}")
    assert all(k.footprint <= E.CAP_BYTES for k in every)
    assert big.footprint <= 100 << 20 and E.REFUSED.footprint < 1 << 20
    assert len({ids(k) for k in E.ALL}) == len(E.ALL) <= 250
    for name, table in E.TABLES.items():
        assert len(table) <= 40 and {k.diag for k in table} == set(E.DIAG_MODES), name
        assert {k.group for k in table} == {name} and all(k.f64 == (name == "f64") for k in table)
        # every shape with every diagonal mode, unless that cross exceeds 40 cases: then every shape has at least one
        # mode, and every mode appears on every engine the table reaches
        modes = {}
        for k in table:
            modes.setdefault((k.n1, k.n2, k.c, k.B), set()).add(k.diag)
        if 3 * len(modes) <= 40:
            assert all(m == set(E.DIAG_MODES) for m in modes.values()), name
            assert len(table) == 3 * len(modes)
        else:
            assert name in ("valu", "mfma") and all(modes.values())
            for inst in {i for k in table for i in E.route(k)["inst"]}:
                assert {k.diag for k in table if inst in E.route(k)["inst"]} == set(E.DIAG_MODES), (name, inst)
    assert {n: len(t) for n, t in E.TABLES.items()} == {"valu": 25, "mfma": 31, "cols": 39, "fused": 30, "f64": 39}


def small_shapes():
    seen, out = set(), []
    for k in E.ALL:
        key = (k.B, k.n1, k.n2, k.c)
        if k.N <= SMALL and key not in seen:
            seen.add(key)
            out.append(k)
    return out


@pytest.mark.parametrize("k", small_shapes(), ids=ids)
def test_the_float64_reference_is_the_int64_einsum(k):
    """... of the same inputs, within the case's bound; the inputs are the integers the bound is derived for, the
    factors are not symmetric, and a transposed factor moves the product."""
    dat = E.case_data(k)
    for name in ("K1", "K2", "v"):
        assert dat[name].dtype == np.float32 and set(np.unique(dat[name]).tolist()) <= {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert set(np.unique(dat["d_full"]).tolist()) <= {1.0, 2.0, 3.0} and set(np.unique(dat["d_const"]).tolist()) <= {1.0, 2.0, 3.0}
    i64 = E.product_int64(dat["K1"], dat["K2"], dat["v"])
    assert i64.dtype == np.int64 and np.array_equal(dat["Kv"], i64.astype(np.float64))
    assert np.array_equal(dat["Kv_t1"], E.product_int64(dat["K1"].transpose(0, 2, 1), dat["K2"], dat["v"]).astype(np.float64))
    assert np.array_equal(dat["Kv_t2"], E.product_int64(dat["K1"], dat["K2"].transpose(0, 2, 1), dat["v"]).astype(np.float64))
    for mode in E.DIAG_MODES:
        ref = E.reference(E.Kron(k.group, k.n1, k.n2, k.c, k.B, mode, k.f64))
        assert np.abs(ref).max() <= k.bound
        assert E.exact(ref.astype(np.float32), ref)
    if k.B > 1:   # members differ, and so do their constant diagonals
        assert not np.array_equal(dat["K1"][0], dat["K1"][1]) or k.n1 == 1
        assert not np.array_equal(dat["v"][0], dat["v"][1]) and dat["d_const"][0] != dat["d_const"][1]


def shapes_once(table):
    seen, out = set(), []
    for k in table:
        key = (k.B, k.n1, k.n2, k.c)
        if key not in seen:
            seen.add(key)
            out.append(k)
    return out


@pytest.mark.parametrize("k", shapes_once(E.ALL + E.MISALIGNED), ids=ids)
def test_no_factor_is_symmetric_and_a_transposed_factor_moves_the_reference(k):
    dat = E.case_data(k)
    for name, n, twin in (("K1", k.n1, "Kv_t1"), ("K2", k.n2, "Kv_t2")):
        Kf = dat[name]
        if n > 1:
            for b in range(k.B):
                assert not np.array_equal(Kf[b], Kf[b].T), (name, b)
            assert not np.array_equal(dat[twin], dat["Kv"]), name
        else:
            assert np.array_equal(dat[twin], dat["Kv"])
    assert np.abs(dat["Kv"]).max() <= 27 * k.N and E.exact(dat["Kv"].astype(np.float32), dat["Kv"])


def test_the_checker_takes_nothing_but_the_reference():
    ref = np.array([[1.0, -25.0], [16777215.0, 3.0]])
    assert E.exact(ref.astype(np.float32), ref) and E.exact(ref.copy(), ref)
    assert not E.exact(np.nextafter(ref.astype(np.float32), np.float32(9)), ref)
    assert not E.exact(ref.astype(np.float32).ravel(), ref)
    bad = ref.astype(np.float32)
    bad[0, 1] = np.nan
    assert not E.exact(bad, ref) and "(0, 1)" in E.mismatches(bad, ref)
    with pytest.raises(AssertionError):
        E.exact(ref.astype(np.float32), ref + float(1 << 24))   # 2^24 + 1: a reference float32 cannot hold
    with pytest.raises(AssertionError):
        E.exact(ref.astype(np.int64), ref)


# ---- coverage ----------------------------------------------------------------------------------------------------------------
def test_every_engine_and_instantiation_is_reached():
    assert {E.route(k)["engine"] for k in E.ALL} == {"valu", "mfma", "cols", "fused", "f64"}
    for name in ("valu", "mfma", "cols", "f64"):
        assert {E.route(k)["engine"] for k in E.TABLES[name]} == {name}, name
    assert {E.route(k)["engine"] for k in E.FUSED} == {"fused", "mfma"}            # (B = 95: below the gate)
    assert {E.route(k, no_fused=True)["engine"] for k in E.FUSED} == {"mfma"}
    assert insts(E.FUSED) >= {("k_kron_fused", ni, ns) for ni, ns in ((8, 4), (8, 0), (4, 2), (4, 0))}
    assert insts(E.MFMA) == {("k_kron_nt_mfma", epi, guard) for epi in (False, True) for guard in (False, True)}
    assert insts(E.COLS) == {("k_kron_cols",), ("k_kron_nt_mfma", False, False), ("k_kron_nt_mfma", False, True)}
    assert insts(E.F64) == {("k64_kron_gemm", True), ("k64_kron_gemm", False)}
    names = set()
    for k in E.ALL:
        names |= set(E.route(k)["kernels"])
    assert names == {"kron_gemm", "kron_gemm_mfma", "kron_fused", "kron_cols", "vec_add_diag"}
    assert [E.route(k)["engine"] for k in E.MISALIGNED] == ["mfma", "mfma", "cols", "fused", "valu"]
    assert E.route(E.MISALIGNED[0])["inst"] != E.route(E.MISALIGNED[1])["inst"]     # aligned and guarded


def test_the_valu_table_sits_on_every_listed_edge():
    t, e = E.VALU, edges(E.VALU)
    assert {k.n1 for k in t} >= {1, 15, 16, 17, 63, 65, 129} and {k.n2 for k in t} >= {1, 13, 17, 63, 65, 66}
    assert {k.c for k in t} >= {1, 2, 5} and {k.B for k in t} == {1, 3}
    assert {(k.n1, k.n2, k.c) for k in t} >= {(64, 64, 65), (68, 64, 65), (65, 68, 1), (64, 66, 1)}
    assert e >= {"row tiles > 1", "p1 column tiles > 1", "p2 column tiles > 1", "p1 ragged BK slab", "p2 ragged BK slab",
                 "n2 c = 63", "n2 c = 64", "n2 c = 65", "p2 sa_c == 1", "p2 sa_c != 1", "sb_c == 1", "inner > 1",
                 "c > 64 on matrix-core factors", "one factor refused by kron_mfma_ok", "B = 1", "B = 3"}
    assert e >= {f"diag {m}" for m in E.DIAG_MODES}
    # more than one row tile with an odd n1 and with c > 64; three row tiles; whole BK slabs as well as ragged ones
    assert any(k.n1 > 64 and k.n1 % 2 for k in t) and any(k.n1 > 64 and k.c > 64 for k in t)
    assert any(E.route(k)["grids"]["pass1"][1] == 3 for k in t) and any(k.n1 % 16 == 0 and k.n2 % 16 == 0 for k in t)
    assert all(not E.route(k)["refused"] for k in t) and E.route(E.REFUSED)["refused"]
    assert E.route(E.REFUSED)["engine"] == "valu" and E.REFUSED.B * E.REFUSED.c == 65552


def test_the_mfma_table_sits_on_every_listed_edge():
    t, e = E.MFMA, edges(E.MFMA)
    aligned = [k for k in t if E.km_aligned(k.n1, k.n2)]
    guarded = [k for k in t if not E.km_aligned(k.n1, k.n2)]
    assert {(k.n1, k.n2) for k in aligned} == {(a, b) for a in (128, 256, 384) for b in (128, 256, 384)}
    assert all(not E.kron_fused_taken(k.B, k.n1, k.n2) for k in t)
    sizes = {64, 68, 124, 132, 192, 252, 260}
    assert {k.n1 for k in guarded} >= sizes and {k.n2 for k in guarded} >= sizes
    assert {(k.n1, k.n2) for k in guarded} >= {(64, 64), (68, 68), (260, 132), (128, 68), (68, 128), (256, 132)}
    assert {k.B for k in aligned} == {1, 7, 8, 9} == {k.B for k in guarded}
    assert e >= {"aligned", "guard", "tiles > 1", "tiles in both directions", "ragged K slab", "one step past a tile",
                 "one step before a tile", "one step past a slab", "half a tile", "mixed aligned / ragged", "Z % 8 != 0",
                 "Z % 8 == 0", "Z < 8", "Z == 8", "Z > 8", "below the gate"}
    for sub in (aligned, guarded):   # the epilogue's three diagonal modes in both instantiations
        assert {k.diag for k in sub} == set(E.DIAG_MODES)


def test_the_cols_table_sits_on_every_listed_edge():
    t, e = E.COLS, edges(E.COLS)
    assert {k.c for k in t if (k.n1, k.n2, k.B) == (64, 64, 1)} == {2, 3, 16, 17, 63, 64}
    for shape in ((64, 68), (68, 68), (128, 128)):
        assert {k.c for k in t if (k.n1, k.n2) == shape} == {3, 17}, shape
    assert {k.B * k.c for k in t} >= {3, 8, 9, 51}
    assert e >= {"LDS > 64 KB", "ld = c", "ld = c + 1", "ragged last block", "a_div with B > 1", "Z % 8 != 0", "Z % 8 == 0",
                 "aligned", "guard", "c = 63", "c = 64"} | {f"cols diag {m}" for m in E.DIAG_MODES}
    assert 64 * 68 == 17 * 256 and 68 * 68 % 256 == 16
    lds = {k.c: E.route(k)["grids"]["lds"] for k in t}
    assert lds[64] == 66560 > 65536 >= lds[63]
    assert {k.diag for k in t if k.c == 64} == set(E.DIAG_MODES)


def test_the_fused_table_sits_on_every_listed_edge():
    t = E.FUSED
    want = {(128, 128, 96): (4, 2), (128, 128, 97): (4, 2), (128, 256, 48): (4, 0), (128, 256, 49): (4, 0),
            (128, 384, 32): (4, 0), (256, 256, 48): (8, 4), (256, 256, 49): (8, 4), (256, 128, 96): (8, 0),
            (256, 384, 32): (8, 0)}
    got = {(k.n1, k.n2, k.B): E.route(k) for k in t}
    assert set(got) == set(want) | {(128, 128, 95)}
    for shape, inst in want.items():
        assert got[shape]["engine"] == "fused" and got[shape]["inst"] == {("k_kron_fused",) + inst}, shape
    assert got[(128, 128, 95)]["engine"] == "mfma" and got[(128, 128, 95)]["kernels"] == {"kron_gemm_mfma": 2}
    for inst in set(want.values()):   # every instantiation meets every diagonal mode
        modes = {k.diag for k in t if E.route(k)["inst"] == {("k_kron_fused",) + inst}}
        assert modes == set(E.DIAG_MODES), inst
    e = edges(t)
    assert e >= {"B % 8 != 0", "B % 8 == 0", "at the gate", "NS = 0 at n2 = 128", "NS = 0 at n2 = 256", "NS = 0 at n2 = 384"}
    # with the switch every case runs the two launches at a batch the aligned table does not have
    assert {E.route(k, no_fused=True)["kernels"] == {"kron_gemm_mfma": 2} for k in t} == {True}
    assert "Z % 8 != 0" in edges(t, no_fused=True) and "Z > 8" in edges(t, no_fused=True)


def test_the_float64_table_sits_on_every_listed_edge():
    t, e = E.F64, edges(E.F64)
    sizes = {1, 15, 16, 17, 31, 32, 33, 65}
    assert {k.n1 for k in t} == sizes == {k.n2 for k in t}
    assert {k.c for k in t} == {1, 2, 7, 8, 9} and {k.B for k in t} == {1, 3}
    assert e >= {"kfast", "kslow", "c = 7", "c = 8", "Q = 31", "Q = 32", "Q = 33", "n = 31", "n = 32", "n = 33", "n = 1",
                 "m tiles > 1", "pass 1: q tiles > 1", "pass 2: q tiles > 1", "ragged kGK slab"}
    for shape in {(k.n1, k.n2, k.c, k.B) for k in t}:
        assert {k.diag for k in t if (k.n1, k.n2, k.c, k.B) == shape} == set(E.DIAG_MODES)
    (a1, a2), (b1, b2) = E.SUM_TERMS
    assert a1 * a2 == b1 * b2 and (a1, a2) != (b1, b2) and set(E.SUM_COLS) == {1, 9}   # kfast and not
    assert 2 * 27 * a1 * a2 + 9 < 1 << 53


def test_the_cg_step_shapes_take_the_routes_they_are_listed_for():
    routes = [E.route(E.Kron("cg", n1, n2, 1, B, "const")) for n1, n2, B in E.CG_STEP]
    assert [r["engine"] for r in routes] == ["mfma", "mfma", "mfma", "fused"]
    assert [("k_kron_nt_mfma", True, g) in r["inst"] for r, g in zip(routes, (False, True, True))] == [True] * 3
    # a dropped or doubled tile moves alpha by at least 1 / (tiles + 1): at most six tiles here, so by 1/7 or more
    tiles = [E.kron_S_dot(n1, n2, 1, 0) for n1, n2, _ in E.CG_STEP]
    assert tiles == [2, 2, 3, 1] and max(tiles) + 1 <= 7
