"""The Lanczos case table (tests/lanczos_cases.py) without a GPU: the oracle's own runs pass the checker in both
precisions, the checker fails on every mutation a wrong kernel would produce -- against the SAME bounds the GPU tests
use -- and the stop conditions the GPU tests rely on hold for the table's inputs."""
import numpy as np
import pytest

import lanczos_cases as lc

NAMES = [c.name for c in lc.CASES]
# what the oracle's own run may show at most, so that FACTOR x its value is a bound below the cap
ORACLE_MAX = {p: lc.CAP[p] / lc.FACTOR for p in ("f32", "f64")}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_passes_the_checker_in_both_precisions(name):
    c = lc.BY_NAME[name]
    for prec in ("f32", "f64"):
        q, t = lc.oracle_run(name, prec)
        if c.steps > 0:
            assert q.shape[-1] == c.steps and t.shape[-1] == c.steps, (name, prec, q.shape)
        vals = lc.oracle_values(name, prec)
        line = f"{name} {prec}: " + " ".join(f"{k}={v:.2e}" for k, v in vals.items())
        print(line)
        assert vals["sym"] == 0.0 and vals["offmin"] >= 0.0, line
        assert ("recon" in vals) == (q.shape[-1] == c.N), line
        for k in lc.BOUNDED:
            if k in vals:
                assert vals[k] <= ORACLE_MAX[prec], line
        assert not lc.violations(vals, lc.bounds(name, prec)), line


def test_route_column_of_the_table_restates_the_host_selection():
    for c in lc.CASES:
        assert lc.expected_route(c) == c.route, c.name
    routes = {c.route for c in lc.CASES}
    assert {"fused", "alpha", "plain4", "scalar", "none"} <= routes
    assert any(c.num_iter == lc.FUSED_Q + 1 and c.route == "fused" for c in lc.CASES)       # nq = 20 = MAXQ
    assert any(c.num_iter == lc.FUSED_Q + 2 and c.route == "plain4" for c in lc.CASES)      # one past it
    for route in ("plain4", "scalar"):  # the _any pair: more than MAX_Q stored vectors
        assert any(c.num_iter > lc.MAX_Q + 1 and c.route == route for c in lc.CASES), route


@pytest.mark.parametrize("shape", lc.F64_SHAPES + (lc.F64_STOP,))
def test_float64_oracle_passes_the_checker(shape):
    rank1 = shape == lc.F64_STOP
    (q, t), vals = lc.f64_oracle(*shape, rank1=rank1)
    line = f"{shape}: " + " ".join(f"{k}={v:.2e}" for k, v in vals.items())
    print(line)
    assert t.shape[-1] == (2 if rank1 else min(shape[2], shape[1])), line
    assert vals["sym"] == 0.0 and vals["offmin"] >= 0.0, line
    for k in lc.BOUNDED:
        if k in vals:
            assert vals[k] <= ORACLE_MAX["f64"], line


# ---- the checker has teeth ---------------------------------------------------------------------------------------------
def _scale_last_alpha(q, t, V):
    t[..., -1, -1] *= 1 + 1e-4


def _scale_last_alpha_1e3(q, t, V):
    t[..., -1, -1] *= 1 + 1e-3


def _scale_mid_beta(q, t, V):
    j = t.shape[-1] // 2
    t[..., j, j + 1] *= 1 + 1e-4
    t[..., j + 1, j] *= 1 + 1e-4


def _scale_one_mirror(q, t, V):
    j = t.shape[-1] // 2
    t[1, 0, j, j + 1] *= 1 + 1e-4


def _drop_last_slice(q, t, V):
    q[2, 1, 260:, 7] = 0  # rows 260..516 of N = 517: the second row slice


def _swap_probe_columns(q, t, V):
    q[[0, 1], 0, :, 5] = q[[1, 0], 0, :, 5]


def _unnormalised_q0(q, t, V):
    q[..., 0] = np.moveaxis(V, -1, 0)


BIG, SMALL = "fused-N517-P4-k21", "fused-N6-P4-k9"
# (what, the fused-shape case it starts from, the mutation).  The quantities are relative to ||A||_2: at N = 517 the
# operator's norm is 78 and the last alpha 1.0, so 1e-4 of it is 1.3e-6 ||A|| -- twice the oracle's own 6.7e-7 and under
# the bound of 8 x that, for any checker whose bound comes from a float32 reference.  The 1e-4 mutation of the last alpha
# therefore starts from the N = 6 fused case (||A|| = 2.8); at N = 517 the check resolves 1e-3.
MUTATIONS = (
    ("last alpha scaled by 1 + 1e-4", SMALL, _scale_last_alpha),
    ("last alpha scaled by 1 + 1e-3", BIG, _scale_last_alpha_1e3),
    ("a mid beta and its mirror scaled by 1 + 1e-4", BIG, _scale_mid_beta),
    ("one of two mirror entries changed", BIG, _scale_one_mirror),
    ("rows of the last slice of one basis vector zeroed", BIG, _drop_last_slice),
    ("two probe columns of one basis vector swapped", BIG, _swap_probe_columns),
    ("q0 left unnormalised", BIG, _unnormalised_q0),
)


@pytest.mark.parametrize("what,name,mutate", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_checker_fails_on_what_a_wrong_kernel_would_write(what, name, mutate):
    assert lc.BY_NAME[name].route == "fused" and lc.BY_NAME[BIG].N == 517
    q, t = (a.copy() for a in lc.oracle_run(name, "f32"))
    bnd = lc.bounds(name)
    assert not lc.violations(lc.check_case(name, q, t), bnd)  # without the mutation: passes
    mutate(q, t, lc.operands(name)["V"])
    vals = lc.check_case(name, q, t)
    bad = lc.violations(vals, bnd)
    print(what, bad, lc.tag(name, vals, lc.oracle_values(name, "f32"), bnd))
    assert bad, (what, vals, bnd)


# ---- the stop conditions the GPU tests rely on ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in lc.STOP_CASES])
def test_rank_one_operator_stops_the_oracle_after_two_vectors(name):
    c = lc.BY_NAME[name]
    o = lc.operands(name)
    assert o["d"] is None and o["C"].shape == (1, c.N, 1) and abs(float((o["C"].astype(np.float64) ** 2).sum()) - 1) < 1e-6
    for prec in ("f32", "f64"):
        q, t = lc.oracle_run(name, prec)
        assert q.shape == (c.P, 1, c.N, 2) and t.shape == (c.P, 1, 2, 2), (name, prec, q.shape, t.shape)


def test_batch_global_case_keeps_the_oracle_going_past_the_exhausted_member():
    c = lc.GLOBAL_STOP
    o = lc.operands(c.name)
    assert not o["C"][0, :, 1:].any() and not o["d"][0].any()  # member 0: u u^T alone
    for prec in ("f32", "f64"):
        q, t = lc.oracle_run(c.name, prec)
        assert q.shape[-1] > 2 and t.shape[-1] == q.shape[-1], (prec, q.shape)
        # member 0 alone stops after two vectors: its beta_1 is rounding noise
        assert abs(t[:, 0, 1, 2]).max() <= 1e-6 < abs(t[:, 1, 1, 2]).min(), (prec, t[:, :, 1, 2])
