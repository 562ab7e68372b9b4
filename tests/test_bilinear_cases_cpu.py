"""The edge cases of the backward contraction kernels and of the SLQ eigensolver without a GPU
(tests/bilinear_cases.py): every case reaches the branch it is listed for, the componentwise bounds
gamma_K * mag hold for a float32 emulation of each kernel's summation order (so they are neither vacuous nor tighter
than the arithmetic allows), and the SLQ bounds hold for an fp64 QL iteration rounded once.  These are conditions on
the inputs and bounds of tests/test_gpu_backward_kernels.py, checked on the references alone; the route labels and the
largest err / bound per family are printed (pytest -s)."""
import numpy as np
import pytest

import bilinear_cases as E


# ---- routes ----------------------------------------------------------------------------------------------------------
def test_every_case_reaches_its_branch():
    for name, table, route in (("dense", E.DENSE_CASES, E.dense_route), ("diag", E.DIAG_CASES, E.diag_route),
                               ("root", E.ROOT_CASES, E.root_route), ("kron", E.KRON_CASES, E.kron_route),
                               ("slq", E.SLQ_CASES, E.slq_route)):
        for case, label in table:
            print(f"route {name} {case}: {route(*case)}")
            assert route(*case) == label, (name, case)


def test_every_route_label_is_reached():
    dense = [E.dense_facts(*c) for c, _ in E.DENSE_CASES]
    assert {f["passes"] for f in dense} == {1, 2, 3}
    assert {f["tiles"] for f in dense} == {1, 2, 3}
    diag = [E.diag_facts(*c) for c, _ in E.DIAG_CASES]
    assert {f["rb"] for f in diag} == {256, 248, 2, 1}
    assert {f["spans"] for f in diag} == {True, False}
    assert {f["strides"] for f in diag} == {1, 2}
    root = [E.root_facts(*c) for c, _ in E.ROOT_CASES]
    launches = [l for f in root for l in f["launches"]]
    assert {l["engine"] for l in launches} == {"mfma1", "mfma2", "valu"}
    assert {l["nw"] for l in launches} == {2, 4}
    assert {l["tiles"] for l in launches} == {1, 8}
    assert {len(f["chunks"]) for f in root} == {1, 2}
    assert {f["S"] for f in root} == {1, 2}


def test_route_facts_the_tables_rely_on():
    # dense: an exact tile with one column in the second pass; 2 x 2 tiles whose edge tile holds one row, three passes
    assert E.dense_facts(2, 64, 65) == {"passes": 2, "dn_last": 1, "tiles": 1, "edge": 64}
    assert E.dense_facts(2, 65, 130) == {"passes": 3, "dn_last": 2, "tiles": 2, "edge": 1}
    # diag: LDS exactly full at D = 8192, refused above; a block of (2, 257, 32) spans the members, none of (2, 256, 2)
    assert E.diag_facts(1, 5, 8192)["rb"] * 8192 == E.BDIAG_LDS and E.BDIAG_LDS // 8193 == 0
    assert E.diag_facts(2, 257, 32)["last"] == 2 and E.diag_facts(2, 256, 2)["strides"] == 1
    # root: D = 62, R = 33 is 2046 pairs and takes phase B to exactly 64000 B with two waves
    assert 62 * 33 == 2046 and E.root_launch_facts(2, 257, 33, 62)["lds_out"] == 64000
    assert E.root_chunks(33, 62) == [(0, 62)]
    # ... R = 48 caps a chunk at 42 columns: 64 = 42 + 22, and 42 columns fill 64 KB with four waves
    assert E.root_chunks(48, 64) == [(0, 42), (42, 22)] and E.root_launch_facts(2, 257, 48, 42)["lds_out"] == 65536
    # ... one member of 515 rows is cut into slices of 260 and 255 rows
    assert E.choose_split(1, 515, 256) == (2, 260)
    # ... 2048 members of 129 rows: eight row blocks per workgroup, one workgroup per member, the second block holds one
    # row and the third starts beyond N
    big = E.root_launch_facts(2048, 129, 8, 4)
    assert (big["tiles"], big["grid_x"], big["nblk"]) == (8, 1, 2) and 129 - 128 == 1
    # ... and alone the same member takes one block per workgroup: its bits are not compared with the batch's
    assert E.root_launch_facts(1, 129, 8, 4)["tiles"] == 1
    # kron: the refusal B D > 65535 of the test; a K of the second stage that is no multiple of the 16-slab
    assert 3856 * 17 == 65552 and (65 * 3) % E.GEMM_BK != 0
    # slq: 65 tridiagonals need a second block of 64 threads
    assert E.slq_route(5, 13, 2, "spd").startswith("M65 blocks2")


def test_inputs_are_independent_draws():
    K1, K2, U, V, *_ = E.kron_inputs((3, 65, 17, 2))
    assert not np.array_equal(K1, np.swapaxes(K1, -1, -2)) and not np.array_equal(K2, np.swapaxes(K2, -1, -2))
    assert not np.array_equal(U, V)
    for t in (K1, K2, U, V):
        assert t.dtype == np.float32


# ---- the bounds hold for the float32 emulation -----------------------------------------------------------------------
def _report(name, ratios):
    worst = max(ratios)
    print(f"emulation {name}: largest err / bound {worst:.3f} over {len(ratios)} comparisons")
    assert 0 < worst <= 1.0, (name, ratios)


def test_dense_bound_holds_for_the_emulation():
    ratios = []
    for case, _ in E.DENSE_CASES:
        U, V, ref, mag = E.dense_inputs(case)
        ratios.append(E.err_over_bound(E.emu_dense(U, V), ref, mag, E.dense_K(*case)))
    _report("dense", ratios)


def test_diag_bound_holds_for_the_emulation():
    for constant in (False, True):
        ratios = []
        for case, _ in E.DIAG_CASES:
            U, V, refs = E.diag_inputs(case)
            ref, mag = refs[constant]
            got = E.emu_diag(U, V, constant)
            assert got.shape == ref.shape
            ratios.append(E.err_over_bound(got, ref, mag, E.diag_K(*case, constant)))
        _report("constant diag" if constant else "diag", ratios)


def test_root_bound_holds_for_the_emulation():
    out_ratios, dot_ratios = [], []
    for case, _ in E.ROOT_CASES:
        Cm, U, V, ref, mag, rd, rd_mag = E.root_inputs(case)
        k_out, k_dot = E.root_K(*case)
        out, dot = E.emu_root(Cm, U, V)
        out_ratios.append(E.err_over_bound(out, ref, mag, k_out))
        dot_ratios.append(E.err_over_bound(dot, rd, rd_mag, k_dot))
    _report("root", out_ratios)
    # (D = 1 makes rowdot a single rounded product: its ratio can be anything up to 1, the others stay far below)
    _report("root rowdot", dot_ratios)


def test_kron_bound_holds_for_the_emulation():
    r1, r2 = [], []
    for case, _ in E.KRON_CASES:
        K1, K2, U, V, ref, mag, _ = E.kron_inputs(case)
        k1, k2 = E.kron_K(*case)
        d1, d2 = E.emu_kron(K1, K2, U, V)
        r1.append(E.err_over_bound(d1, ref[0], mag[0], k1))
        r2.append(E.err_over_bound(d2, ref[1], mag[1], k2))
    _report("kron dK1", r1)
    _report("kron dK2", r2)


def test_kron_bound_sees_a_transposed_factor():
    """With the non-symmetric factors the oracle evaluated with K2^T (K1^T) is far outside the bound around the oracle
    itself -- the symmetric factors of cases.kron_factors cannot tell the two apart."""
    for case, _ in E.KRON_CASES:
        B, n1, n2, D = case
        *_, ref, mag, swapped = E.kron_inputs(case)
        k1, k2 = E.kron_K(*case)
        if n2 > 1:
            assert E.err_over_bound(swapped[0], ref[0], mag[0], k1) > 100
        if n1 > 1:
            assert E.err_over_bound(swapped[1], ref[1], mag[1], k2) > 100


def test_dense_bound_sees_a_lost_pass():
    """U V^T of (2, 65, 130) contracted over its first 64 columns only -- what a lost second and third pass would leave
    -- misses the bound by orders of magnitude; 5e-3 of the maximum norm is what the suite compared it at before."""
    case = (2, 65, 130)
    U, V, ref, mag = E.dense_inputs(case)
    lost = E.orc.bilinear_derivative_dense(U[..., :64].astype(np.float64), V[..., :64].astype(np.float64))
    assert E.err_over_bound(lost, ref, mag, E.dense_K(*case)) > 1e3


# ---- SLQ -------------------------------------------------------------------------------------------------------------
def test_negative_cases_have_the_stated_gap():
    for case, _ in E.SLQ_CASES:
        lam = E.slq_reference(case)["lam"]
        if case[3] == "negative":
            assert ((lam <= -0.1).sum(-1) == 1).all() and (np.abs(lam) >= 0.1).all()
        else:
            assert (lam >= 0.1).all(), case
        if case[3] == "padded":  # the padding is an identity block: T - 7 eigenvalues are exactly 1
            assert ((lam == 1.0).sum(-1) == case[2] - E.SLQ_PAD_FROM).all()
        if case[3] == "repeated":
            assert (lam == 1.5).all()


def test_slq_bounds_hold_for_an_fp64_ql_rounded_once():
    worst = {}
    for case, _ in E.SLQ_CASES:
        t = E.slq_matrices(case).astype(np.float64)
        P, B, T, _ = case
        lam, vec = np.empty((P, B, T)), np.empty((P, B, T, T))
        for p in range(P):
            for b in range(B):
                lam[p, b], vec[p, b] = E.ql_implicit64(t[p, b])
        own = E.slq_check(case, *E.slq_from_eigh64(case, lam, vec))
        lib = E.slq_check(case, *E.slq_from_eigh64(case, *np.linalg.eigh(t)))
        for res in (own, lib):
            for k, v in res.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("emulation slq: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert set(worst) == {"evals", "recon", "orth", "logdet"}
    assert all(0 < v <= 1.0 for v in worst.values()), worst


def test_slq_check_rejects_an_unmasked_negative_eigenvalue():
    case = (2, 2, 12, "negative")
    lam, vec = np.linalg.eigh(E.slq_matrices(case).astype(np.float64))
    with pytest.raises(AssertionError):
        E.slq_check(case, lam.astype(np.float32), vec.astype(np.float32), None)
