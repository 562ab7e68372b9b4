"""The edge cases of the 1-D Toeplitz / SKI kernels without a GPU (tests/ski_edge_cases.py): the restated launch
arithmetic equals the library's own sizers, every branch the cases are listed for is reached by a table row, every row
keeps float32 sums exact, and the inputs are not blind: a reference with one deliberate mistake per branch is told from
the right one by the checker.  These are conditions on the inputs of tests/test_gpu_ski_edges.py, checked on the
references alone."""
import numpy as np
import pytest

import ski_edge_cases as E
from linear_operator_amd import _hip


# ---- the mirrors -------------------------------------------------------------------------------------------------------
def test_splits_are_the_ones_the_shapes_were_chosen_for():
    want = {(1, 1): (1, 1, 256, 1), (1, 2): (1, 1, 256, 2), (1, 255): (1, 1, 256, 255), (1, 256): (1, 1, 256, 256),
            (1, 257): (2, 2, 256, 1), (1, 513): (3, 3, 256, 1), (1, 517): (3, 3, 256, 5), (40, 1030): (5, 3, 512, 6),
            (64, 1030): (5, 2, 768, 262), (171, 517): (3, 1, 768, 517)}
    assert set(want) == set(E.TZ_SHAPES)
    for shape, split in want.items():
        assert E.tz_split(*shape) == split, shape
        assert E.bil_split(*shape) == split, shape   # (the two splits are the same arithmetic today)
    # what tests/test_gpu_ski.py reaches: one slice, or eight slices that are exact multiples of 256
    assert E.tz_split(1, 37) == (1, 1, 256, 37)
    assert E.tz_split(3, 2048) == (8, 8, 256, 256) and E.tz_split(1, 16384) == (64, 8, 2048, 2048)


def test_mirrors_equal_the_library_sizers():
    lib = _hip.load()
    for B, M in E.TZ_SHAPES:
        for c in E.tz_cols(B):
            assert int(lib.lo_toeplitz_workspace_bytes(B, M, c)) == E.toeplitz_workspace_bytes(B, M, c), (B, M, c)
    rows = [row[2:] for row in E.INTERP_CASES] + [E.WRAP[2:]] + [(2 * E.BCAST_P, *row[3:]) for row in E.INTERP_CASES]
    rows += list(E.SKI_SHAPES)
    for B, M, N, J in rows:
        assert int(lib.lo_interp_plan_bytes(B, N, J, M)) == E.plan_bytes(B, N, J, M), (B, M, N, J)
        assert int(lib.lo_interp_t_workspace_bytes(B, N, J, M)) == E.plan_bytes(B, N, J, M), (B, M, N, J)
    lay, end = E.plan_layout(3, 100, 4, 255)
    assert [lay[k][0] for k in ("ptr", "cur", "tmp", "ids")] == [0, 3072, 6144, 11008] and end == 11008 + 4800


# ---- every branch is reached ---------------------------------------------------------------------------------------------
def test_toeplitz_cases_reach_every_branch():
    splits = {s: E.tz_split(*s) for s in E.TZ_SHAPES}
    # several k slices, the last one short
    assert any(KS > 1 and last < kchunk and last % 256 for _, KS, kchunk, last in splits.values())
    assert {512, 768} <= {kchunk for _, _, kchunk, _ in splits.values()}
    # kchunk > 256 with a partial last k tile inside a slice that is not the only one
    assert any(KS > 1 and kchunk > 256 and last % 256 for _, KS, kchunk, last in splits.values())
    # one slice of several k tiles, the last of 5
    assert splits[(171, 517)] == (3, 1, 768, 517) and 517 % 256 == 5
    # the row guard i < M with more than one row block
    assert any(RB > 1 and M % 256 for (_, M), (RB, *_) in splits.items())
    chunks = [ch for c in E.TZ_COLS_ONE for ch in E.column_chunks(c)]
    assert {cb for _, _, cb in chunks} == set(E.TZ_CB)
    for cb in (4, 8, 16, 24, 32):
        assert any(CB == cb and cc < CB for _, cc, CB in chunks), cb
    assert any(col0 >= 32 and cc > 1 for col0, cc, _ in chunks)
    assert any(col0 == 64 for col0, _, _ in chunks)   # a third chunk
    assert E.column_chunks(65) == [(0, 32, 32), (32, 32, 32), (64, 1, 1)] and E.column_chunks(40)[1] == (32, 8, 8)
    assert E.column_chunks(17) == [(0, 17, 24)] and E.column_chunks(3) == [(0, 3, 4)]
    # the batched shapes keep a cc < CB launch and a second chunk
    assert E.column_chunks(3)[0][2] == 4 and E.column_chunks(33)[1] == (32, 1, 1)
    # k_tz_reduce makes a second pass at (64, 1030, 33), and LO_DIAG_CONST runs with more than one member
    assert E.wraps(64, 1030, 1, 1, 33)["k_tz_reduce"] and 64 * 1030 * 33 > E.ELEM_CAP
    assert E.wraps(171, 517, 1, 1, 33)["k_tz_reduce"] and not E.wraps(40, 1030, 1, 1, 33)["k_tz_reduce"]
    assert len(set(E.const_diag(64).tolist())) == 6 and np.all(E.const_diag(171)[1:] != E.const_diag(171)[:-1])


def test_lag_correlation_cases_reach_every_branch():
    splits = {s: E.bil_split(*s) for s in E.TZ_SHAPES}
    M_of = {M for _, M in E.TZ_SHAPES}
    assert {1, 2, 255, 256, 257} <= M_of and 1 in E.BIL_S
    assert any(ichunk > 256 for _, _, ichunk, _ in splits.values())
    # a last i slice that ends inside a tile while later rows exist for the shifted windows: ua / va masked by i < ie,
    # uw / vw by i < M (not the last slice), and a short last slice
    assert any(KI > 1 and last % 256 for _, KI, _, last in splits.values())
    assert any(KI > 1 and ichunk % 256 == 0 and ichunk > 256 for _, KI, ichunk, _ in splits.values())


def test_interpolation_cases_reach_every_branch():
    assert E.scatter_mode(7) == "wave" and E.scatter_mode(8) == "lane" and {7, 8} <= set(E.INTERP_C)
    assert set(E.BCAST_C) == {7, 8}
    longest, empties, dup, outside_seen = 0, 0, False, set()
    for name, pattern, B, M, N, J in E.INTERP_CASES:
        idx, _ = E.interp_case(name)
        seg = E.segment_lengths(idx, M)
        longest = max(longest, int(seg.max()))
        empties += int((seg == 0).sum())
        if pattern == "clustered":
            assert set(np.unique(seg).tolist()) == {N} | ({0} if M > J else set()), name
        if pattern == "empty":
            assert (seg == 0).mean() > 0.95
        if pattern == "duplicate":
            assert np.all(idx[..., 0] == idx[..., 1])
            dup = True
        if pattern == "outside":
            bad = idx[~E.in_range(idx, M)]
            outside_seen |= {int(x) - (M if x >= M else 0) for x in np.unique(bad)}
            assert not E.in_range(idx[:, 0], M).any()            # a row of nothing else
            assert 0.15 < (~E.in_range(idx, M)).mean() < 0.45
    assert {n for _, p, _, _, n, _ in E.INTERP_CASES if p == "clustered"} == {1, 64, 65, 200}
    assert longest == 200 and empties > 0 and dup
    assert outside_seen == {-1, 0, 5, -(1 << 40)}   # -1, M, M + 5, -2^40
    assert {M for _, _, _, M, _, _ in E.INTERP_CASES} == {1, 255, 256, 1000}
    assert {J for *_, J in E.INTERP_CASES} == {1, 4, 16} and {B for _, _, B, *_ in E.INTERP_CASES} == {1, 3}


def test_the_wrap_case_wraps_every_loop():
    _, _, B, M, N, J = E.WRAP
    w1, w16 = E.wraps(B, M, N, J, 1), E.wraps(B, M, N, J, 16)
    assert w1["k_csr_count"] and w1["k_csr_fill"] and w1["k_interp_vgrad"] and w1["k_csr_sort"]
    assert w1["k_interp_t_wave"] and w16["k_interp_t_lane"] and w16["k_interp"]
    # ... and nothing else in the tables does
    for _, _, B, M, N, J in E.INTERP_CASES:
        for c in E.INTERP_C:
            assert not any(E.wraps(B, M, N, J, c).values())


# ---- float32 sums stay exact ---------------------------------------------------------------------------------------------
def test_every_row_keeps_float32_sums_exact():
    worst = 0
    for B, M in E.TZ_SHAPES:
        worst = max(worst, 9 * M + 9, 2 * max(E.BIL_S) * M * 9)   # units of 1: the product + d o v; the correlation
    for name, _, B, M, N, J in E.INTERP_CASES + (E.WRAP,):
        for members in (None, 2 * E.BCAST_P):
            if name == "wrap" and members:
                continue
            idx, _ = E.interp_case(name, members)
            seg = int(E.segment_lengths(idx, M).max())
            worst = max(worst, 4 * 3 * J, 4 * 3 * seg, 9 * max(E.VGRAD_S))   # units of 1/4: W u, W^T v; of 1: the gradient
    for shape in E.SKI_SHAPES:
        for outside in (False, True):
            k = E.ski_case(*shape, outside)
            v = np.full((shape[0], shape[2], 1), 3.0)   # |v| <= 3 in every column
            for ri, rv in ((k["ri"], k["rv"]), (k["li"], k["lv"])):
                bound = E.ski_ref(k["t"], k["li"], k["lv"], ri, rv, v, k["d_full"], "full", absolute=True).max()
                print(f"SKI {shape} outside={outside}: 16 sum |terms| = {16 * bound:.0f}")
                worst = max(worst, 16 * bound)   # units of 1/16
    print(f"largest sum of absolute terms: {worst:.0f} units of {E.LIMIT}")
    assert worst < E.LIMIT


# ---- the references and the checker themselves -------------------------------------------------------------------------------
def test_references_agree_with_their_definitions():
    u, v, ref = E.bil_case(1, 257, 2)
    assert np.array_equal(ref, E.bil_ref_definition(u, v))
    u, v, ref = E.bil_case(40, 1030, 5)
    assert np.array_equal(ref[::13], E.bil_ref_definition(u[::13], v[::13]))
    # W^T v and W u through the dense W of one member
    name = "outside-M1000"
    idx, vals = E.interp_case(name)
    _, M, N, J = E.case_shape(name)
    W = np.zeros((N, M))
    ok = E.in_range(idx[1], M)
    np.add.at(W, (np.repeat(np.arange(N), J)[ok.ravel()], idx[1][ok]), vals[1][ok].astype(np.float64))
    v, u = E.operand(name, "v", N, 7), E.operand(name, "u", M, 7)
    assert np.array_equal(E.wt_ref(idx, vals, v, M)[1], W.T @ v[1]) and np.array_equal(E.w_ref(idx, vals, u)[1], W @ u[1])
    ptr, ids = E.csr_ref(idx, M)
    assert ptr[1, -1] == ok.sum() and sorted(ids[1].tolist()) == np.flatnonzero(ok.ravel()).tolist()
    flat = idx[1].ravel()
    assert np.all(np.diff(flat[ids[1]]) >= 0) and np.all((np.diff(flat[ids[1]]) > 0) | (np.diff(ids[1]) > 0))


def test_the_checker_takes_nothing_but_the_reference():
    ref = np.array([[1.0, -2.5], [0.0625, 3.0]])
    assert E.exact(ref.astype(np.float32), ref)
    assert not E.exact(np.nextafter(ref.astype(np.float32), np.float32(9)), ref)
    assert not E.exact(ref.astype(np.float32).ravel(), ref)
    bad = ref.astype(np.float32)
    bad[0, 1] = np.nan
    assert not E.exact(bad, ref) and "(0, 1)" in E.mismatches(bad, ref)
    with pytest.raises(AssertionError):
        E.exact(ref.astype(np.float32), ref + 2.0 ** -30)   # a reference float32 cannot hold
    with pytest.raises(AssertionError):
        E.exact(ref, ref)                                   # float64 is not what a kernel returns


# ---- the inputs make each mistake visible --------------------------------------------------------------------------------
def _lag_shifted_at_a_tile_boundary():
    """The tile of rows 256.. and k 0..255 of (1, 517) reads t[255] for the lag 256 (one entry of its window)."""
    t, u, _, ref = E.tz_case(1, 517, 1)
    T = E.toeplitz_dense(t[0])
    i = np.arange(256, 512)
    T[i, i - 256] = t[0, 255]
    return (T @ u[0])[None], ref


def _last_k_slice_dropped():
    t, u, _, ref = E.tz_case(1, 517, 1)
    _, KS, kchunk, _ = E.tz_split(1, 517)
    T = E.toeplitz_dense(t[0])
    T[:, (KS - 1) * kchunk:] = 0
    return (T @ u[0])[None], ref


def _k_mask_removed():
    """The last slice of (40, 1030) reads on to the end of its k tile: rows of the next member's u (nothing behind the
    last member), with the lags |i - k| < M the window still holds."""
    B, M, c = 40, 1030, 3
    t, u, _, ref = E.tz_case(B, M, c)
    _, KS, kchunk, last = E.tz_split(B, M)
    kend = (KS - 1) * kchunk + E.ceil_div(last, 256) * 256
    assert kend > M
    out = ref.copy()
    i, k = np.arange(M)[:, None], np.arange(M, kend)[None, :]
    lag = np.abs(i - k)
    for b in range(B - 1):
        Tx = np.where(lag < M, t[b].astype(np.float64)[np.minimum(lag, M - 1)], 0.0)
        out[b] += Tx @ u[b + 1, :kend - M].astype(np.float64)
    return out, ref


def _column_beyond_cc_written():
    """CB = 4 serving cc = 3 writes its fourth accumulator (0): the first column of the next row."""
    _, _, _, ref = E.tz_case(1, 255, 3)
    assert E.column_chunks(3) == [(0, 3, 4)]
    out = ref.copy()
    out[0, 1:, 0] = 0.0
    return out, ref


def _outside_index_clamped():
    name = "outside-M1000"
    idx, vals = E.interp_case(name)
    _, M, N, _ = E.case_shape(name)
    v = E.operand(name, "v", N, 1)
    return E.wt_ref(np.clip(idx, 0, M - 1), vals, v, M), E.wt_ref(idx, vals, v, M)


def _outside_index_clamped_in_the_gather():
    name = "outside-M255-J16"
    idx, vals = E.interp_case(name)
    _, M, _, _ = E.case_shape(name)
    u = E.operand(name, "u", M, 8)
    return E.w_ref(np.clip(idx, 0, M - 1), vals, u), E.w_ref(idx, vals, u)


def _segment_cut_at_64():
    name = "clustered-N65"
    idx, vals = E.interp_case(name)
    _, M, N, _ = E.case_shape(name)
    v = E.operand(name, "v", N, 1)
    return E.wt_ref(idx[:, :64], vals[:, :64], v[:, :64], M), E.wt_ref(idx, vals, v, M)


def _duplicates_collapsed():
    name = "duplicate-M255"
    idx, vals = E.interp_case(name)
    B, M, N, J = E.case_shape(name)
    v = E.operand(name, "v", N, 7)
    out = np.zeros((B, M, 7))
    for b in range(B):
        for n in range(N):
            out[b][idx[b, n]] += vals[b, n].astype(np.float64)[:, None] * v[b, n]   # (a buffered +=: one per point)
    return out, E.wt_ref(idx, vals, v, M)


def _const_diag_read_per_row():
    B, M, c = 40, 1030, 3
    _, u, _, ref = E.tz_case(B, M, c)
    d = E.const_diag(B)
    per_row = d[(np.arange(B * M) % B)].reshape(B, M)   # dd[e / c] kept inside the B values there are
    return ref + E.diag_term(per_row, u, "full"), ref + E.diag_term(d, u, "const")


def _a2_kept_at_lag_0():
    u, v, ref = E.bil_case(1, 257, 1)
    out = ref.copy()
    out[:, 0] *= 2
    return out, ref


MUTATIONS = {"tz(1,517,1): a lag shifted by one at a tile boundary": _lag_shifted_at_a_tile_boundary,
             "tz(1,517,1): the last k slice dropped": _last_k_slice_dropped,
             "tz(40,1030,3): the k < ke mask removed": _k_mask_removed,
             "tz(1,255,3): a column at q >= cc written": _column_beyond_cc_written,
             "interp_t outside-M1000: an outside index clamped": _outside_index_clamped,
             "interp outside-M255-J16: an outside index clamped": _outside_index_clamped_in_the_gather,
             "interp_t clustered-N65: a segment cut at 64 entries": _segment_cut_at_64,
             "interp_t duplicate-M255: duplicates collapsed": _duplicates_collapsed,
             "toeplitz kind (40,1030,3): the CONST diagonal read per row": _const_diag_read_per_row,
             "bilinear(1,257,1): a2 kept at lag 0": _a2_kept_at_lag_0}


@pytest.mark.parametrize("name", MUTATIONS)
def test_the_checker_fails_on_a_reference_with_one_mistake(name):
    wrong, right = MUTATIONS[name]()
    assert E.exact(right.astype(np.float32), right)
    assert not E.exact(wrong.astype(np.float32), right), name
    print(name, "->", E.mismatches(wrong, right, limit=2))


def test_neighbouring_lags_differ_in_every_column():
    for B, M in E.TZ_SHAPES:
        t = E.tz_case(B, M, 1)[0]
        assert np.all(t != 0) and np.all(t[:, 1:] != t[:, :-1])
