"""The MINRES case table (tests/minres_cases.py) without a GPU: what makes a fixed-step comparison valid holds for every
case, and the checker -- against the SAME bounds the GPU test uses -- reports what a wrong kernel would write.

Conditions, asserted for every case: the float32 oracle's own figures are at most 5e-4 / 8 (the cap can only tighten the
8 x rule); the float64 oracle equals the independent Krylov minimiser (float64 cases: 1e-11; every unpreconditioned case
with k <= 12: an eighth of its bound); the iterate still moves by 100 x the bound per step (an off-by-one step count or
a stale vector cannot hide; after step k >= N there is no next iterate to compare with, and `wrapper-cap-N6`, which
runs past the Krylov space on purpose, is exempt and pinned by its iteration count); the float64 conv of a stopping case
is 4 x away from the tolerance at every check.  A seed or a spectrum that misses one is changed; the bounds are not."""
import numpy as np
import pytest

import minres_cases as mc
from oracle import lo_oracle as orc

f32, f64 = np.float32, np.float64
ORACLE_MAX = mc.CAP / mc.FACTOR


def cases_where(pred):
    return [n for n in mc.RUNNABLE if pred(mc.BY_NAME[n])]


# ---- the table itself ----------------------------------------------------------------------------------------------------
def test_table_reaches_the_slices_columns_and_partial_counts_it_is_built_for():
    by_group = lambda g: [c for c in mc.CASES if c.group == g]  # noqa: E731
    splits = {c.name: mc.choose_split(c.B, c.N) for c in by_group("slices")}
    assert {S for S, _ in splits.values()} == {1, 2, 4}, splits
    short = {n: c_N - (S - 1) * rows for n, (S, rows) in splits.items() for c_N in [mc.BY_NAME[n].N] if S > 1}
    assert all(0 < v for v in short.values()) and any(v < mc.choose_split(2, mc.BY_NAME[n].N)[1] for n, v in short.items())
    assert splits["slices-N517-k3"] == (2, 260) and splits["slices-N1027-k3"] == (4, 260) and splits["slices-N1030-k3"] == (4, 260)
    assert splits["slices-N255-k3"][0] == 1 and splits["slices-N260-k3"][0] == 1
    assert {c.k for c in by_group("slices") if c.N == 517} >= {2, 3, 9, 10, 11}
    assert any(c.k == c.N for c in by_group("slices") if c.N == 3) and any(c.k == c.N for c in by_group("slices") if c.N == 6)
    cols = sorted(c.c for c in by_group("columns"))
    assert cols == [1, 2, 4, 5, 64, 85, 86, 128, 129, 255, 256, 257]
    assert [256 // c for c in (85, 86, 128, 129, 256)] == [3, 2, 2, 1, 1] and 256 - 2 * 86 == 84  # nrs, the idle threads
    assert all(mc.choose_split(c.B, c.N)[0] == 2 for c in by_group("columns") + by_group("rhs") + by_group("stopping"))
    # the operands group: every rule for the number of q . K q partials, each different from S where it can be
    rules = {c.name: (mc.s_dot(c), mc.choose_split(c.B, c.N)[0]) for c in by_group("operands")}
    assert rules["operand-dense-mfma"] == ((9, True), 2) and rules["operand-dense-valu16"] == ((33, True), 2)
    assert rules["operand-dense-small"] == ((7, True), 1) and rules["operand-dense-valu32"] == ((9, True), 1)
    assert {mc.dense_s_dot(c.B, c.N, c.c)[1] for c in by_group("operands") if c.kind == "dense"} == {"mfma", "valu16", "valu32"}
    assert rules["operand-kron-3x5"] == ((1, False), 1) and rules["operand-kron-128x128"] == ((1, True), 64)
    assert rules["operand-toeplitz"][0] == (2, False) and rules["operand-sum"][0] == (2, False)
    assert rules["operand-closure"][0] == (2, False) and rules["operand-tensor"][0] == (9, True)
    assert {c.precond[1] for c in by_group("preconditioners") if isinstance(c.precond, tuple)} == {1, 5, 8}
    assert {c.N for c in by_group("preconditioners")} == {517, 1030}
    assert all(np.all(mc.operands(c.name)["shifts"] != 0) for c in by_group("preconditioners"))
    assert set(mc.REFUSED) == {f"slices-N{N}-k1" for N in (3, 6, 255, 260, 517, 1027, 1030)} | {"columns-c257", "f64-grid-refused"}
    g = mc.BY_NAME["f64-grid-refused"]
    assert g.Q * g.B > 65535
    assert 10 <= len(mc.F64_CASES) <= 14


def test_shift_cases_are_what_their_names_say():
    sh = mc.operands("shifts-Q5-member-B3")["shifts"]
    assert sh.shape == (5, 3) and len(set(sh.ravel().tolist())) == 15
    assert mc.operands("shifts-Q15-shared")["shifts"].shape == (15,)
    assert mc.operands("shifts-Q1-member")["shifts"].shape == (1, 2) and mc.operands("shifts-Q1-shared")["shifts"].shape == (1,)
    for name in ("shifts-value-1", "f64-dense-value-1"):
        c, o = mc.BY_NAME[name], mc.operands(name)
        assert c.value == -1.0
        A = mc.matmul(name, f64)(np.broadcast_to(np.eye(c.N), (c.B, c.N, c.N)).copy())
        assert o["shifts"].min() > np.linalg.eigvalsh(A).max() + 0.5, name
    c, o = mc.BY_NAME["shifts-indefinite"], mc.operands("shifts-indefinite")
    lam = np.linalg.eigvalsh(mc.matmul(c.name, f64)(np.broadcast_to(np.eye(c.N), (c.B, c.N, c.N)).copy()))
    sigma = float(o["shifts"][0])
    assert sigma < 0 and np.all(np.abs(lam + sigma) >= 0.3), float(np.abs(lam + sigma).min())
    assert np.all((lam + sigma).min(-1) < 0) and np.all((lam + sigma).max(-1) > 0)
    assert np.all(np.abs(lam + float(o["shifts"][1])) >= 0.3)


# ---- the conditions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.RUNNABLE)
def test_conditions_of_a_valid_fixed_step_comparison(name):
    c = mc.BY_NAME[name]
    x, info, conv = mc.reference(name)
    bnd = mc.bounds(name)
    assert info.iterations == c.k, (name, info.iterations)
    assert info.converged == (name in ("stop-at-10", "stop-at-20", "f64-dense-stop-at-10")), name
    assert np.all(np.isfinite(x))
    if c.dtype == "f32":
        vals, (x32, info32, conv32) = mc.oracle_values(name), mc.oracle_f32(name)
        print(f"{name}: oracle float32 err {vals['err']:.2e} resid {vals['resid']:.2e}; bounds {bnd['err']:.2e} {bnd['resid']:.2e}")
        assert vals["err"] <= ORACLE_MAX and vals["resid"] <= ORACLE_MAX and vals["zeros"] == 0, (name, vals["err"], vals["resid"])
        assert (info32.iterations, info32.converged) == (info.iterations, info.converged), name
        assert not mc.violations(vals, bnd), name  # the unmutated float32 run passes
        assert all(mc.FLOOR <= b <= mc.CAP for b in bnd.values())
    if c.opts.get("still_moving", True):
        mv = mc.movement(name)
        print(f"{name}: moves {mv:.2e} per step, {mv / max(bnd.values()):.0f} x the bound")
        assert mv >= mc.MOVING * max(bnd.values()), (name, mv, bnd)
    if c.precond is None and c.k <= mc.KRYLOV_MAX_K and c.tol == 0.0:
        e = float(mc.rel_err(x, mc.krylov(name)).max())
        print(f"{name}: oracle float64 against the Krylov minimiser {e:.2e}")
        assert e <= (1e-11 if c.dtype == "f64" else min(bnd.values()) / 8), (name, e)
        if c.dtype == "f64":  # an independent computation passes the float64 bound
            assert not mc.violations(mc.check(name, mc.krylov(name)), bnd), name


@pytest.mark.parametrize("name", mc.STOPPING + ("rhs-zero-column-tol1",))
def test_stopping_cases_sit_four_times_away_from_their_tolerance(name):
    c = mc.BY_NAME[name]
    _, info, conv = mc.reference(name)
    assert sorted(conv) == list(range(10, c.k + 1, 10)), (name, conv)
    if name == "rhs-zero-column-tol1":
        assert np.isnan(conv[10]) and info.iterations == c.max_iter + 2 == 12 and not info.converged
        return
    for at, v in conv.items():
        assert max(v / c.tol, c.tol / v) >= 4.0, (name, at, v, c.tol)
        assert (v < c.tol) == (at == c.k and info.converged), (name, at, v)
        assert mc.conv_bound(name, at) < 1e-3, (name, at, mc.conv_bound(name, at))  # (cannot reach across the tolerance)


# ---- the checker bites ---------------------------------------------------------------------------------------------------
def run_altered(name, shifts=None, op=None):
    """The float32 oracle's k steps of a case with other shifts or another operator."""
    c, o = mc.BY_NAME[name], mc.operands(name)
    sh = o["shifts"] if shifts is None else np.asarray(shifts, f32)
    with np.errstate(all="ignore"):
        x, _ = orc.minres(op or mc.operator(name, f32), o["rhs"], shifts=sh, value=c.value, max_iter=c.k - 2,
                          preconditioner=mc.preconditioner(name, f32), tolerance=0.0)
    return x.reshape(c.Q, c.B, c.N, c.c)


def caught(name, x, what):
    bad = mc.violations(mc.check(name, x), mc.bounds(name))
    assert "err" in bad or "zeros" in bad, (name, what, bad)
    return bad


def good(name):
    return np.array(mc.oracle_f32(name)[0])


def test_member_0_shifts_used_for_every_member_is_caught():
    name = "shifts-Q5-member-B3"
    sh = mc.operands(name)["shifts"]
    caught(name, run_altered(name, np.repeat(sh[:, :1], 3, axis=1)), "member 0's shifts")
    name = "shifts-Q1-member"
    sh = mc.operands(name)["shifts"]
    caught(name, run_altered(name, np.repeat(sh[:, :1], 2, axis=1)), "member 0's shifts")


def test_shifts_read_transposed_is_caught():
    name = "shifts-Q5-member-B3"
    sh = mc.operands(name)["shifts"]
    caught(name, run_altered(name, sh.reshape(-1).reshape(3, 5).T), "[Q, B] read as [B, Q]")


@pytest.mark.parametrize("name", cases_where(lambda c: c.dtype == "f32" and c.opts.get("still_moving", True)))
def test_a_neighbouring_iterate_is_caught(name):
    c = mc.BY_NAME[name]
    for j in (c.k - 1, c.k + 1):
        if j < 1 or (j > c.k and c.k >= c.N):
            continue
        caught(name, mc._steps(name, "f32", j), f"x_{j} for x_{c.k}")


@pytest.mark.parametrize("name", ["slices-N517-k3", "slices-N1027-k2", "slices-N1030-k3", "slices-N517-k10", "columns-c256"])
def test_stale_rows_at_the_end_of_the_last_slice_are_caught(name):
    c = mc.BY_NAME[name]
    x = good(name)
    x[..., -7:, :] = mc._steps(name, "f32", c.k - 1)[..., -7:, :]
    caught(name, x, "the last 7 rows left at x_(k-1)")


@pytest.mark.parametrize("name", ["slices-N517-k3", "rhs-scales", "columns-c5"])
def test_a_column_scaled_by_its_neighbours_norm_is_caught(name):
    c = mc.BY_NAME[name]
    nrm = np.sqrt((mc.operands(name)["rhs"].astype(f64) ** 2).sum(-2))  # [B, c]
    x = good(name).astype(f64)
    x = x * (np.roll(nrm, -1, axis=-1) / nrm)[None, :, None, :]
    caught(name, x, "rhs_norm of column j + 1")


def test_value_applied_to_the_shift_is_caught():
    for name in ("shifts-value2.5", "shifts-value-1"):
        c = mc.BY_NAME[name]
        caught(name, run_altered(name, c.value * mc.operands(name)["shifts"]), "value x shift")


@pytest.mark.parametrize("name", ["slices-N517-k3", "slices-N1030-k3", "slices-N1027-k2"])
def test_the_diagonal_dropped_on_the_last_slice_is_caught(name):
    c, o = mc.BY_NAME[name], mc.operands(name)
    S, rows = mc.choose_split(c.B, c.N)
    d = o["d"].copy()
    d[:, (S - 1) * rows:] = 0.0
    caught(name, run_altered(name, op=lambda v: orc.matvec_lowrank_diag(o["C"], d, v)), "a slice's part of alpha")


@pytest.mark.parametrize("name", cases_where(lambda c: c.group != "columns" or c.c in (1, 256)))
def test_a_relative_perturbation_of_1e_3_of_one_solution_is_caught(name):
    c = mc.BY_NAME[name]
    x = np.array(mc.reference(name, "f32" if c.dtype == "f32" else "f64")[0]).astype(f64)
    x[c.Q - 1, 0, :, c.c // 2] *= 1 + 1e-3
    caught(name, x, "1e-3 of one (shift, member, column)")


def test_a_value_in_a_zero_column_is_caught():
    for name in ("rhs-zero-column", "rhs-zero-column-tol1"):
        x = good(name)
        assert np.all(x[:, -1, :, -1] == 0)
        x[1, -1, 300, -1] = 1e-30
        assert mc.violations(mc.check(name, x), mc.bounds(name)) == ["zeros"]
        x[1, -1, 300, -1] = np.nan
        assert mc.violations(mc.check(name, x), mc.bounds(name)) == ["zeros"]
