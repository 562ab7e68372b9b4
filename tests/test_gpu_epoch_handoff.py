"""The headline solve without its clearing launch (csrc/lo_rspace3.hip): k_cg_rspace3 keeps what its workgroups
share -- error word, member / close counters, exchange and close granules -- in a buffer the library owns and clears once;
launches are told apart by a host-assigned tag base (exchange granules) and epoch (close granules).

  * consecutive solves repeat bit for bit and never clear the buffer;
  * shapes that change the group size and the granule layout from launch to launch meet each other's leftovers;
  * an injected hand-off timeout, and solves on other engines in between, leave the next resident solve bit-equal;
  * the counters wrap by clearing the buffer.
"""
import os

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

from linear_operator_amd import kernels as K  # noqa: E402


@pytest.fixture(autouse=True)
def _form_on_second_use():
    old = K.EIGFORM_AFTER_USES
    K.EIGFORM_AFTER_USES = 1
    K.set_onchip_cg(True)  # (ends any cool-down another test may have left)
    yield
    K.EIGFORM_AFTER_USES = old
    K.inject_resident_timeouts(0)
    K.set_onchip_cg(True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Case:
    """One operator with its root-form preconditioner, already on the diagonal form."""

    def __init__(self, seed, B, N, R):
        C, d, rhs = cases.lowrank_diag(seed, B, N, R, 1)
        self.C, self.d = C, d
        self.desc = K.lowrank_diag_descriptor(dev(C), dev(d))
        L, perm = K.pivoted_cholesky(self.desc, 15)
        self.L = L
        self.pre = K.precond_build(L, dev(d), constant_diag=False, root=self.desc.A0, perm=perm)
        self.rhs = dev(rhs)
        self.solve()  # first use: dense R-space form
        self.solve()  # second use: the cache gets the diagonal form
        assert torch.is_tensor(self.pre.RSD)

    def solve(self):
        return K.cg_solve(self.desc, self.rhs, precond=self.pre, tolerance=1e-4)

    def solve_owned(self):
        """A solve that must run k_cg_rspace3 on the library's buffer: (result, buffer was cleared in front of it)."""
        s0 = K.resident_handoff_debug()
        res = self.solve()
        e = K.cg_last_executed()
        s1 = K.resident_handoff_debug()
        assert e["resident"] and e["rspace"] == "resident" and e["rspace_diag"] and e["lean"], e
        assert e["streaming_iterations"] == 0, e
        assert s1["launches"] == s0["launches"] + 1, "the solve did not run on the library's hand-off buffer"
        return res, s1["clears"] - s0["clears"]

    def reference(self):
        """The same solve right after a forced clear of the buffer."""
        K.resident_handoff_debug(force_clear=True)
        res, cleared = self.solve_owned()
        assert cleared == 1
        return res


def test_consecutive_headline_solves_repeat_and_never_clear():
    cs = Case(8101, 64, 8192, 32)
    first = cs.reference()
    for i in range(300):
        res, cleared = cs.solve_owned()
        assert cleared == 0, f"solve {i} cleared the buffer"
        assert torch.equal(res.x, first.x), f"solve {i} differs"
        assert res.iterations == first.iterations and res.mean_residual == first.mean_residual


def test_alternating_shapes_meet_each_others_granules():
    shapes = [(64, 8192, 32), (8, 4096, 16), (64, 1000, 8), (8, 8192, 32), (64, 4096, 8), (8, 1000, 16)]
    cs = [Case(8200 + i, B, N, R) for i, (B, N, R) in enumerate(shapes)]
    refs = [c.reference() for c in cs]
    for rnd in range(4):
        order = list(range(len(cs))) if rnd % 2 == 0 else list(reversed(range(len(cs))))
        for i in order:
            res, cleared = cs[i].solve_owned()
            assert cleared == 0
            assert torch.equal(res.x, refs[i].x), (rnd, shapes[i])
            assert res.iterations == refs[i].iterations and res.mean_residual == refs[i].mean_residual


def test_injected_timeout_leaves_the_buffer_dirty_and_the_next_launch_clears_it():
    cs = Case(8301, 64, 8192, 32)
    ref = cs.reference()
    s0 = K.resident_status()
    K.inject_resident_timeouts(1)
    hit = cs.solve()  # the resident launch starts with its error word set: redone on the streaming engine
    e = K.cg_last_executed()
    s1 = K.resident_status()
    assert not e["resident"] and e["streaming_iterations"] >= 11, e
    assert s1["timeouts"] == s0["timeouts"] + 1 and s1["cooldown"] > 0
    assert hit.iterations == ref.iterations
    for _ in range(s1["cooldown"] - 1):  # the cool-down: fall-back engine
        cs.solve()
        assert not K.cg_last_executed()["resident"]
    res, cleared = cs.solve_owned()  # re-armed
    assert cleared == 1, "the launch behind a timed-out one must clear the buffer"
    assert torch.equal(res.x, ref.x)
    s2 = K.resident_status()
    assert s2["timeouts"] == s0["timeouts"] + 1 and s2["cooldown"] == 0
    res, cleared = cs.solve_owned()
    assert cleared == 0 and torch.equal(res.x, ref.x)


def test_other_engines_in_between():
    cs = Case(8401, 64, 8192, 32)
    ref = cs.reference()
    # 17 columns with 16 tridiagonals: the all-column R-space form / lockstep engines on the caller's workspace
    Cm, dm, rhs17 = cases.lowrank_diag(8402, 64, 8192, 32, 17)
    r17 = K.cg_solve(cs.desc, dev(rhs17), precond=cs.pre, n_tridiag=16, tolerance=1e-4)
    e = K.cg_last_executed()
    assert e["resident"] and not e["rspace_diag"], e
    assert torch.isfinite(r17.x).all()
    res, cleared = cs.solve_owned()
    assert cleared == 0 and torch.equal(res.x, ref.x)
    # a Q-only preconditioner: the second-generation / streaming engines
    preq = K.precond_build(cs.L, dev(cs.d), constant_diag=False)
    rq = K.cg_solve(cs.desc, cs.rhs, precond=preq, tolerance=1e-4)
    e = K.cg_last_executed()
    assert e["rspace"] != "resident", e
    assert torch.isfinite(rq.x).all()
    res, cleared = cs.solve_owned()
    assert cleared == 0 and torch.equal(res.x, ref.x)
    # the dense form of the same kernel family (clears the caller's workspace, leaves the library's buffer alone)
    os.environ["LO_RS_NO_DIAG"] = "1"
    try:
        s0 = K.resident_handoff_debug()
        cs.solve()
        assert not K.cg_last_executed()["rspace_diag"]
        assert K.resident_handoff_debug()["launches"] == s0["launches"]
    finally:
        del os.environ["LO_RS_NO_DIAG"]
    res, cleared = cs.solve_owned()
    assert cleared == 0 and torch.equal(res.x, ref.x)


@pytest.mark.parametrize("which", ["tag", "epoch"])
def test_counter_wrap_around_clears_the_buffer(which):
    cs = Case(8501, 64, 8192, 32)
    ref = cs.reference()
    B = 64
    if which == "tag":  # a launch takes B + 2 tags; the limit is 0xfff00000
        K.resident_handoff_debug(next_tag=0xFFF00000 - 4 * (B + 2) - 7)
    else:               # epochs are 29-bit: the limit is 0x1ffffff0
        K.resident_handoff_debug(next_epoch=0x1FFFFFF0 - 4)
    cleared_at = []
    for i in range(10):
        res, cleared = cs.solve_owned()
        assert torch.equal(res.x, ref.x), f"solve {i} around the wrap differs"
        if cleared:
            cleared_at.append(i)
    assert len(cleared_at) == 1 and 2 <= cleared_at[0] <= 5, cleared_at
    st = K.resident_handoff_debug()
    assert st["next_tag"] < 0x1000 * (B + 2) and st["next_epoch"] < 0x1000, st


def test_clear_handoff_switch_takes_the_callers_workspace(monkeypatch):
    cs = Case(8601, 64, 8192, 32)
    ref = cs.reference()
    monkeypatch.setenv("LO_OC_CLEAR_HANDOFF", "1")
    s0 = K.resident_handoff_debug()
    res = cs.solve()
    e = K.cg_last_executed()
    assert e["resident"] and e["rspace_diag"], e
    assert K.resident_handoff_debug()["launches"] == s0["launches"], "the switch must keep the solve off the library's buffer"
    assert torch.equal(res.x, ref.x)
    monkeypatch.delenv("LO_OC_CLEAR_HANDOFF")
    res, cleared = cs.solve_owned()
    assert cleared == 0 and torch.equal(res.x, ref.x)
