"""The edge cases of the SKI grid kind without a GPU (tests/ski_grid_edge_cases.py): every product case reaches the
branch of `grid_axis` it is listed for, and every pivoted Cholesky case is an input on which fp32 rounding cannot flip a
pivot.  These are conditions on the inputs of tests/test_gpu_ski_grid_edges.py, checked on the references alone; the
figures are printed (pytest -s)."""
import numpy as np
import pytest

import ski_grid_edge_cases as E
from make_golden_ski_grid import PC_GAP, PC_RANK, kron_dense64, pivot_gaps64


def test_every_product_case_reaches_its_branch():
    reached = set()
    for grid, c, B, labels in E.PRODUCT_CASES:
        route = E.expected_route(grid, c, B)
        print(f"route {grid} c={c} B={B}: {' | '.join(route)}")
        assert route == labels, (grid, c, B)
        for label in route:
            reached |= E.route_kinds(label)
    assert reached == E.ROUTE_KINDS, sorted(E.ROUTE_KINDS ^ reached)


def test_route_facts_the_table_relies_on():
    # the divisor search of (13, 5, 3), c = 2 starts above the divisor it ends on: the loop decrements
    assert E.shared_lines_start(3, 2, 65) == 42 and E.expected_route((13, 5, 3), 2, 2)[2] == "line_shared(13)"
    # ... and never did in the shapes of tests/test_gpu_ski_grid.py
    assert E.shared_lines_start(8, 2, 1) == 1 and E.shared_lines_start(4, 2, 30) == 30
    # the 63 / 64 boundary between the two lane mappings
    assert E.expected_route((2, 1000), 63, 1)[1].startswith("line")
    assert E.expected_route((2, 1000), 64, 1)[1] == "inner2"
    # a chunked line stages at most kGridStage floats, a shared group at most one workgroup's worth
    for grid, c, B, _ in E.PRODUCT_CASES:
        inner = c
        for Mk in grid[::-1]:
            if inner < E.TILE and Mk * inner >= E.THREADS:
                assert min(Mk, E.STAGE // inner) * inner <= E.STAGE
            inner *= Mk


def test_kron_apply64_is_the_dense_kronecker_product():
    cols, u = E.product_inputs((6, 5, 4), 2, 3)
    for b in range(3):
        member = [t[b] for t in cols]
        ref = kron_dense64(member) @ u[b].astype(np.float64)
        assert np.abs(E.kron_apply64(member, u[b]) - ref).max() <= 1e-12 * np.abs(ref).max()


def test_pivchol64_generalises_the_golden_recurrence():
    """With W_l = W_r and every index inside the grid, pivchol64 is pivot_gaps64 of the golden generator."""
    _, cols, li, lv, _, _, _ = E.pivot_case("g3_shared")
    piv, gaps = pivot_gaps64(cols, li[0], lv[0], PC_RANK)
    p64, L64, g64, _ = E.pivot_reference64("g3_shared")[0]
    assert np.array_equal(piv, p64) and np.allclose(gaps, g64, rtol=1e-12, atol=0)
    # L L^T reproduces the pivot rows of the true matrix
    M = int(np.prod([t.shape[-1] for t in cols]))
    W = E._w_dense_dropping64(li[0], lv[0], M)
    A = W @ kron_dense64(cols) @ W.T
    assert np.abs((L64 @ L64.T)[p64][:, p64] - A[p64][:, p64])[np.triu_indices(PC_RANK, 1)].max() <= 1e-12 * A.max()


@pytest.mark.parametrize("name", E.PIVOT_CASES)
def test_pivot_case_cannot_flip_in_fp32(name):
    _, cols, li, lv, ri, rv, _ = E.pivot_case(name)
    for b, (p64, L64, gaps, low) in enumerate(E.pivot_reference64(name)):
        p32, L32 = E.pivchol32(E.member_cols(cols, b), li[b], lv[b], ri[b], rv[b], PC_RANK)
        level = np.abs(L32 - L64).max() / np.abs(L64).max()
        print(f"pivots {name}[{b}]: smallest gap {gaps.min():.3e}, smallest diagonal {low:.3e}, "
              f"|L32 - L64| / max |L64| = {level:.3e}, pivots {p64.tolist()}")
        assert gaps.min() >= PC_GAP, gaps
        assert low > 0.0
        assert np.array_equal(p32, p64)


def test_out_of_grid_case_touches_a_pivot_row_and_a_row_never_selected():
    grid, _, li, _, ri, _, shared = E.pivot_case("g3_out_of_grid")
    M = int(np.prod(grid))
    assert not shared
    bad_l, bad_r = np.argwhere((li < 0) | (li >= M)), np.argwhere((ri < 0) | (ri >= M))
    assert len(bad_l) == 2 and len(bad_r) == 2
    assert sorted(li[tuple(bad_l.T)].tolist()) == [-1, M] and sorted(ri[tuple(bad_r.T)].tolist()) == [-1, M]
    piv = set(E.pivot_reference64("g3_out_of_grid")[0][0].tolist())
    rows = set(bad_l[:, 1].tolist()) | set(bad_r[:, 1].tolist())
    assert rows & piv and rows - piv
    assert set(bad_l[:, 1].tolist()) & piv and set(bad_r[:, 1].tolist()) & piv  # (one on either side, in fact)
    # the edits change the factor: the case is not the shared one again
    assert not np.array_equal(E.pivot_reference64("g3_out_of_grid")[0][1], E.pivot_reference64("g3_shared")[0][1])


def test_separate_right_weights_are_distinct_values():
    _, _, li, lv, ri, rv, shared = E.pivot_case("g2_separate")
    assert not shared and ri is not li and np.array_equal(ri, li) and not np.array_equal(rv, lv)
    for name in ("g3_members", "g2_separate"):
        cols = E.pivot_case(name)[1]
        assert all(t.ndim == 2 and not np.allclose(t[0] / t[0, 0], t[1] / t[1, 0]) for t in cols)  # not only a scale


def test_measured_rounding_level():
    """PC_ROUNDING is the largest |L32 - L64| / max |L64| over the cases and members, rounded up to two digits."""
    worst = 0.0
    for name in E.PIVOT_CASES:
        _, cols, li, lv, ri, rv, _ = E.pivot_case(name)
        for b, (_, L64, _, _) in enumerate(E.pivot_reference64(name)):
            _, L32 = E.pivchol32(E.member_cols(cols, b), li[b], lv[b], ri[b], rv[b], PC_RANK)
            worst = max(worst, np.abs(L32 - L64).max() / np.abs(L64).max())
    print(f"measured fp32 rounding level {worst:.3e}, PC_ROUNDING {E.PC_ROUNDING:.1e}")
    assert worst <= E.PC_ROUNDING <= 1.1 * worst


def test_engine_operator_is_positive_definite():
    _, cols, _, _, d, A = E.engine_case()
    for b in range(2):
        ev = np.linalg.eigvalsh(0.5 * (A[b] + A[b].T))
        print(f"engine operator [{b}]: eigenvalues {ev[0]:.3f} .. {ev[-1]:.1f}")
        assert ev[0] >= 0.5 - 1e-9 and np.abs(A[b] - A[b].T).max() <= 1e-12 * ev[-1]
    assert all(not np.allclose(t[0] / t[0, 0], t[1] / t[1, 0]) for t in cols)
