"""The closing pass of k_cg_rspace3's iteration chain (csrc/lo_rspace3.hip, DESIGN 4.16, profiles/r18): what the last
iteration does behind its x update -- the c update, r.z, beta, the residual norm -- enters only the member's records.
The tree forms the norm in workgroup 0's owning wave alone: in place for a group's final member, at the NEXT member's top
for every other one (deferred, profiles/r12).  A build that also ended the chain of every other wave at the x update and
deferred r.z and beta was measured slower (profiles/r18) and is not in the tree; these are the checks it was held to, and
any later change of the closing pass has to pass them: they do not depend on where the pass runs.

Which of the two a member gets depends on how many groups the launch has and on the direction it walks the members in,
never on the member: a group takes member `grp` first and then the members it draws, and a member is deferred exactly
when its group goes on to another one.  So every shape is solved on the whole device and on a quarter of the groups
(LO_OC_RESERVE_CUS=192), walking forward and in reverse, through the session and through the general path
(LO_CG_NO_SESSION), at max_iter 1, 2, 3 and the default.  The plan gives a solve to the resident kernels only from
max_iter = 11 on (cg_plan, csrc/lo_cg.hip), so max_iter = 1, 2, 3 run on the streaming engine; the kernel's own closing
pass is the first, the second, the third -- another wave owns it each time -- when the first possible stop is:
floor_max_iter = 1, 2, 3 under a tolerance that every member meets there (1e3), so that x and the records are the
kernel's.  Both are run.  Shapes (B, N, R); groups on the whole device / on a quarter:

  (3, 256, 8)      one workgroup per member, 512 / 128 groups: in place only
  (9, 1000, 16)    one workgroup per member, ragged rows: in place only
  (65, 1000, 8)    one workgroup per member, ragged rows: in place only
  (67, 8192, 32)   the headline member shape, 64 / 16 groups: 3 / 51 members deferred
  (131, 1000, 8)   (beyond the issue's list) 128 groups on a quarter: three members deferred without a group exchange
  (40, 4096, 16)   (beyond the issue's list) four workgroups per member, 128 / 32 groups: 0 / 8 members deferred

x, the fp32 mean of the members' residual norms (summed in member order from the records the closing pass stores) and
every other field of the result are compared bit for bit between all of these; copies of one system get one solution;
x meets the fp64 Woodbury solution within 1e-4 at the default max_iter (the bound of tests/test_gpu_eigform.py for this
engine); an all-zero member, a NaN right-hand side at a budget of one iteration and a right-hand side inside span(C)
give the same flags and take the same fall-back whatever the placement.  cg_solve exposes no per-member record and no state of a
continued solve (a continuation repeats the first pass with its state on another engine); a solve whose tolerance the
resident iterations cannot reach is compared between the placements all the same: the records decide that it goes on.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import cases
import test_gpu_early_ticket as et
import test_gpu_rs3_member_path as mp

from linear_operator_amd import kernels as K  # noqa: E402

gpu = pytest.mark.gpu

ISSUE_SHAPES = [(3, 256, 8), (9, 1000, 16), (65, 1000, 8), (67, 8192, 32)]
SHAPES = ISSUE_SHAPES + [(131, 1000, 8), (40, 4096, 16)]
# (kind, k): max_iter = k as the issue names it; "floor": the kernel's own iteration count k; None: the default
BUDGETS = [("max_iter", 1), ("max_iter", 2), ("max_iter", 3), ("floor", 1), ("floor", 2), ("floor", 3), None]


def budget_id(b):
    return "default" if b is None else f"{b[0]}_{b[1]}"


def budget_kw(b):
    if b is None:
        return {"tolerance": 1e-4}
    return {"max_iter": b[1], "tolerance": 1e-4} if b[0] == "max_iter" else {"floor_max_iter": b[1], "tolerance": 1e3}


PLACEMENTS = [(path, grid, walk) for path in ("session", "general") for grid in ("whole", "quarter")
              for walk in ("forward", "reverse")]

_form_on_second_use = et._form_on_second_use  # (autouse: switches, injected time-outs and peers restored)


@pytest.fixture(autouse=True)
def _placement_restored():
    keep = {n: os.environ.get(n) for n in ("LO_CG_NO_SESSION", "LO_OC_RESERVE_CUS")}
    yield
    for n, v in keep.items():
        os.environ.pop(n, None)
        if v is not None:
            os.environ[n] = v
    if torch.cuda.is_available():
        K.resident_order_debug(0)


@contextmanager
def placed(path, grid, walk):
    os.environ.pop("LO_CG_NO_SESSION", None)
    os.environ.pop("LO_OC_RESERVE_CUS", None)
    if path == "general":
        os.environ["LO_CG_NO_SESSION"] = "1"
    if grid == "quarter":
        os.environ["LO_OC_RESERVE_CUS"] = "192"
    K.resident_order_debug(2 if walk == "reverse" else 1)
    try:
        yield
    finally:
        os.environ.pop("LO_CG_NO_SESSION", None)
        os.environ.pop("LO_OC_RESERVE_CUS", None)
        K.resident_order_debug(0)


class System:
    """One operator with its root-form preconditioner on the diagonal form, and one right-hand side."""

    def __init__(self, seed, B, N, R):
        self.shape = (B, N, R)
        self.C, self.d, self.rhs_host = cases.lowrank_diag(seed, B, N, R, 1)
        self.desc = K.lowrank_diag_descriptor(et.dev(self.C), et.dev(self.d))
        L, perm = K.pivoted_cholesky(self.desc, 15)
        self.pre = K.precond_build(L, et.dev(self.d), constant_diag=False, root=self.desc.A0, perm=perm)
        self.pre.ensure_eigform()
        assert torch.is_tensor(self.pre.RSD), self.pre.rsd_refused
        self.rhs = et.dev(self.rhs_host)
        self._runs = {}

    def solve(self, rhs, budget, placement, **over):
        """(result, executed plan, groups of the launch) under one placement."""
        kw = dict(budget_kw(budget), **over)
        with placed(*placement):
            res = K.cg_solve(self.desc, rhs, precond=self.pre, **kw)  # (no right-hand side here makes it raise)
            torch.cuda.synchronize()
            return res, K.cg_last_executed(), K.resident_start_debug()["ngroups"]

    def runs(self, budget):
        """The plain right-hand side under every placement, solved once per (system, budget)."""
        if budget not in self._runs:
            self._runs[budget] = {p: self.solve(self.rhs, budget, p) for p in PLACEMENTS}
        return self._runs[budget]


_systems = {}


def system(shape):
    if shape not in _systems:
        _systems[shape] = System(9500 + SHAPES.index(shape), *shape)
    return _systems[shape]


def bits(x):
    return x.contiguous().view(torch.int32)  # (NaN compares equal to itself)


def fields(res):
    f = (res.iterations, res.matvecs, res.tolerance_reached, res.nan_detected, res.skipped)
    return f + (np.float32(res.mean_residual).tobytes(),)


def assert_same(a, b, what):
    (ra, ea, _), (rb, eb, _) = a, b
    assert torch.equal(bits(ra.x), bits(rb.x)), f"{what}: x differs"
    assert fields(ra) == fields(rb), (what, fields(ra), fields(rb))
    assert {k: ea[k] for k in ("resident", "rspace", "rspace_diag", "resident_iterations", "streaming_iterations")} == \
           {k: eb[k] for k in ("resident", "rspace", "rspace_diag", "resident_iterations", "streaming_iterations")}, what


def on_the_headline_kernel(e):
    return e["resident"] and e["rspace"] == "resident" and e["rspace_diag"]


@gpu
@pytest.mark.parametrize("budget", BUDGETS, ids=budget_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_placements_and_paths_agree_bit_for_bit(shape, budget):
    B, N, R = shape
    runs = system(shape).runs(budget)
    ref = runs[PLACEMENTS[0]]
    print(f"{shape} {budget_id(budget)}: iterations {ref[0].iterations} resident {ref[1]['resident_iterations']} "
          f"streaming {ref[1]['streaming_iterations']} mean residual {ref[0].mean_residual:.6e} groups "
          f"{ref[2]} / {runs[('session', 'quarter', 'forward')][2]}")
    for p, run in runs.items():
        assert_same(run, ref, p)
    assert not ref[0].nan_detected and torch.isfinite(ref[0].x).all()
    if budget is not None and budget[0] == "max_iter":  # (below the resident kernels' threshold: the streaming engine)
        assert not ref[1]["resident"] and ref[0].iterations == budget[1], ref[1]
        return
    for p, run in runs.items():
        assert on_the_headline_kernel(run[1]), (p, run[1])
        if budget is not None:
            assert run[1]["resident_iterations"] == budget[1] and run[1]["streaming_iterations"] == 0, (p, run[1])
            assert run[0].iterations == budget[1] and run[0].tolerance_reached, (p, fields(run[0]))
    whole, quarter = ref[2], runs[("session", "quarter", "forward")][2]
    assert quarter * 4 == whole, (whole, quarter)
    if shape == (67, 8192, 32):
        assert (whole, quarter) == (64, 16)  # three members deferred on the whole device, 51 on a quarter
    assert runs[("general", "quarter", "reverse")][2] == quarter


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_x_meets_the_closed_form(shape):
    cs = system(shape)
    res = cs.runs(None)[PLACEMENTS[0]][0]
    ex = et.woodbury(cs.C, cs.d, cs.rhs_host)
    err = float(((res.x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
    print(f"{shape}: max relative error against fp64 Woodbury {err:.3e}, tolerance reached {res.tolerance_reached}")
    assert res.tolerance_reached
    assert err < 1e-4, err


@gpu
@pytest.mark.parametrize("budget", BUDGETS, ids=budget_id)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_copies_of_one_system_get_one_solution(shape, budget):
    """B copies of one system: a deferred member and a final one hold the same numbers, so they must get the same x --
    the x of a three-copy batch, where every member is its group's final one."""
    B, N, R = shape
    many, three = mp.copies(B, N, R), mp.copies(3, N, R)
    kw = budget_kw(budget)
    headline = budget is None or budget[0] == "floor"
    x3 = K.cg_solve(three.desc, three.rhs, precond=three.pre, **kw).x
    for grid in ("whole", "quarter"):
        for walk in ("forward", "reverse"):
            with placed("session", grid, walk):
                res = K.cg_solve(many.desc, many.rhs, precond=many.pre, **kw)
                assert on_the_headline_kernel(K.cg_last_executed()) == headline, K.cg_last_executed()
            assert torch.equal(res.x, res.x[:1].expand_as(res.x)), (grid, walk, "copies of one system got different solutions")
            # (on the streaming engine the kernels are chosen by the batch size and add in another order: no such property)
            assert not headline or torch.equal(res.x[0], x3[0]), (grid, walk, "the solution differs from the three-copy batch")


def special_right_hand_sides(cs):
    B, N, R = cs.shape
    w = np.random.default_rng(9700 + B).standard_normal((B, R, 1)).astype(np.float32)
    zero = cs.rhs.clone()
    zero[1] = 0
    zero[B - 1] = 0
    nan = cs.rhs.clone()
    nan[1, 7, 0] = float("nan")
    nan[B - 1, N - 1, 0] = float("nan")
    return {"span": et.dev(cs.C @ w), "zero": zero, "nan": nan}


# What the parent commit returns for each special right-hand side and budget, the same at every shape below:
# (iterations, matvecs, tolerance_reached, nan_detected, skipped) and (resident, rspace, rspace_diag, resident
# iterations, streaming iterations) of the executed plan.  Nothing raises.
#   * an all-zero member: the plain solve's fields, on the headline kernel;
#   * NaN, first possible stop at iteration 1: the headline kernel's closing pass is its first product's, and its NaN
#     flag (deferred or in place) is what sets nan_detected; NaN at max_iter = 1: the streaming engine stops at once;
#   * inside span(C): the dense form on the resident engine (rspace_diag off), converged.
PARENT_OUTCOME = {
    ("zero", ("floor", 1)): ((1, 1, True, False, False), (True, "resident", True, 1, 0)),
    ("zero", None): ((11, 11, True, False, False), (True, "resident", True, 11, 0)),
    ("nan", ("floor", 1)): ((1, 1, False, True, False), (True, "resident", True, 1, 0)),
    ("nan", ("max_iter", 1)): ((0, 0, False, True, False), (False, "none", False, 0, 1)),
    ("span", None): ((11, 11, True, False, False), (True, "resident", False, 11, 0)),
    ("span", ("floor", 1)): ((1, 1, True, False, False), (True, "resident", False, 1, 0)),
}


@gpu
@pytest.mark.parametrize("shape", ISSUE_SHAPES + [(131, 1000, 8)], ids=lambda s: "x".join(map(str, s)))
def test_zero_nan_and_span_members_whatever_the_placement(shape):
    """Members 1 and B - 1 carry the special right-hand side: on a quarter of the device the first is deferred at the
    last two shapes, the second is its group's final member wherever a launch walks forward."""
    cs = system(shape)
    B = shape[0]
    rhs = special_right_hand_sides(cs)
    for (name, budget), (want_fields, want_plan) in PARENT_OUTCOME.items():
        runs = {p: cs.solve(rhs[name], budget, p) for p in PLACEMENTS}
        ref = runs[PLACEMENTS[0]]
        res, e, _ = ref
        plan = (bool(e["resident"]), e["rspace"], bool(e["rspace_diag"]), e["resident_iterations"], e["streaming_iterations"])
        print(f"{shape} {name} {budget_id(budget)}: {fields(res)[:5]} {plan} mean residual {res.mean_residual}")
        for p, run in runs.items():
            assert_same(run, ref, (name, budget, p))
        assert fields(res)[:5] == want_fields, (name, budget, fields(res)[:5])
        assert plan == want_plan, (name, budget, e)
        if name == "zero":
            assert torch.count_nonzero(res.x[1]) == 0 and torch.count_nonzero(res.x[B - 1]) == 0
            assert torch.isfinite(res.x).all()
            plain = cs.runs(budget)[PLACEMENTS[0]][0]
            keep = [i for i in range(B) if i not in (1, B - 1)]
            assert torch.equal(res.x[keep], plain.x[keep]), "a zero member changed its neighbours"
        elif name == "span":
            assert torch.isfinite(res.x).all()
    # the solve behind them is the plain one again
    assert_same(cs.solve(cs.rhs, None, PLACEMENTS[0]), cs.runs(None)[PLACEMENTS[0]], "the solve behind the special ones")


@gpu
@pytest.mark.parametrize("shape", [(67, 8192, 32), (40, 4096, 16)], ids=lambda s: "x".join(map(str, s)))
def test_a_solve_that_goes_on_behind_the_resident_iterations(shape):
    """A tolerance the resident iterations cannot reach: the records of the closing pass (deferred or in place) decide
    that the solve goes on; the first pass is then repeated with its state on the root-form engine and continued on the
    streaming one (cg_plan, `lean`).  The decision and the continuation do not depend on the placement."""
    cs = system(shape)
    runs = {p: cs.solve(cs.rhs, None, p, tolerance=1e-9) for p in PLACEMENTS}
    ref = runs[PLACEMENTS[0]]
    print(f"{shape} tolerance 1e-9: {fields(ref[0])[:5]} {ref[1]}")
    for p, run in runs.items():
        assert_same(run, ref, p)
    assert torch.isfinite(ref[0].x).all()
