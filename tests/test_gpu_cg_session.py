"""Native solve sessions of the headline solve (lo_cg_session, csrc/lo_cg.hip): `cg_solve` sends a single
column on a cache that carries the diagonal form through a session that did the per-call set-up once.  The general path
(LO_CG_NO_SESSION=1: the code every solve ran before) is the reference throughout -- results are compared bit for bit.

Shapes (B, N, R): (3, 256, 8) a group of one workgroup at the minimum N; (5, 1500, 16) a group of two whose last wave's
rows are clamped; (70, 2500, 32) more members than the 64 resident groups, so a group draws a second member.
"""
import gc
import os
import sys
from contextlib import contextmanager

if __name__ == "__main__":  # (run as the capture test's child: what conftest.py puts on the path for the suite)
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), os.path.join(_here, "golden")]

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

from linear_operator_amd import kernels as K  # noqa: E402

SHAPES = [(3, 256, 8), (5, 1500, 16), (70, 2500, 32)]
SWITCHES = ("LO_CG_NO_SESSION", "LO_OC_NO_RSPACE", "LO_RS_NO_DIAG")


@pytest.fixture(autouse=True)
def _clean_gate():
    for n in SWITCHES:
        os.environ.pop(n, None)
    K.inject_resident_timeouts(0)
    K.set_onchip_cg(True)  # (ends any cool-down another test may have left, forgets the lean misses)
    gc.collect()
    yield
    for n in SWITCHES:
        os.environ.pop(n, None)
    K.inject_resident_timeouts(0)
    K.set_onchip_cg(True)


@contextmanager
def env(name, on=True):
    if on:
        os.environ[name] = "1"
    try:
        yield
    finally:
        os.environ.pop(name, None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


class Case:
    """One operator, its root-form preconditioner with the diagonal form built explicitly, four right-hand sides."""

    def __init__(self, seed, B, N, R):
        C, d, _ = cases.lowrank_diag(seed, B, N, R, 1)
        self.C, self.d = C, d
        self.desc = K.lowrank_diag_descriptor(dev(C), dev(d))
        self.L, self.perm = K.pivoted_cholesky(self.desc, 15)
        self.pre = self.build()
        g = np.random.default_rng(seed + 1)
        self.rhs = [dev(g.standard_normal((B, N, 1)).astype(np.float32)) for _ in range(4)]

    def build(self, need_q=True):
        pre = K.precond_build(self.L, dev(self.d), constant_diag=False, root=self.desc.A0, perm=self.perm, need_q=need_q)
        pre.ensure_eigform()
        assert torch.is_tensor(pre.RSD), pre.rsd_refused
        return pre

    def solve(self, i=0, rhs=None, **kw):
        kw.setdefault("tolerance", 1e-4)
        res = K.cg_solve(self.desc, self.rhs[i] if rhs is None else rhs, precond=self.pre, **kw)
        return res, K.cg_last_executed()


def fields(res):
    return (res.iterations, res.matvecs, res.tolerance_reached, res.nan_detected, res.skipped, res.mean_residual)


def same(a, b):
    """(CGResult, executed plan) of the two paths: x bit for bit, every field, the plan."""
    (ra, ea), (rb, eb) = a, b
    assert torch.equal(ra.x, rb.x)
    assert ra.t_mat is None and rb.t_mat is None
    fa, fb = fields(ra), fields(rb)
    assert fa[:5] == fb[:5] and (fa[5] == fb[5] or (np.isnan(fa[5]) and np.isnan(fb[5]))), (fa, fb)
    assert ea == eb, (ea, eb)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_session_against_general_path(shape):
    cs = Case(9100 + shape[0], *shape)
    live0 = K.cg_sessions_live()
    runs = {}
    for mode in ("session", "general"):
        with env("LO_CG_NO_SESSION", mode == "general"):
            uses0, out = cs.pre.rs_uses, []
            for i in range(4):
                h0 = K.resident_handoff_debug()
                out.append(cs.solve(i))
                h1 = K.resident_handoff_debug()
                assert h1["launches"] == h0["launches"] + 1, (mode, i)
                assert h1["clears"] == h0["clears"], (mode, i)
            runs[mode] = (out, cs.pre.rs_uses - uses0)
        if mode == "session":
            assert K.cg_sessions_live() == live0 + 1
    for a, b in zip(runs["session"][0], runs["general"][0]):
        same(a, b)
        assert a[1]["rspace"] == "resident" and a[1]["rspace_diag"] and a[1]["lean"] and a[1]["streaming_iterations"] == 0
    assert runs["session"][1] == runs["general"][1] == 4
    assert not torch.equal(runs["session"][0][0][0].x, runs["session"][0][1][0].x)  # (four different right-hand sides)


def general(cs, i=0, **kw):
    with env("LO_CG_NO_SESSION"):
        return cs.solve(i, **kw)


def test_what_ends_a_session():
    live0 = K.cg_sessions_live()
    cs = Case(9201, 5, 1500, 16)
    ref = general(cs)
    same(cs.solve(), ref)
    assert K.cg_sessions_live() == live0 + 1
    # another tolerance, another max_iter: sessions of their own in the cache's small LRU, results as the general path
    same(cs.solve(tolerance=1e-3), general(cs, tolerance=1e-3))
    same(cs.solve(max_iter=500), general(cs, max_iter=500))
    same(cs.solve(), ref)
    assert live0 + 1 <= K.cg_sessions_live() <= live0 + 4
    for k in range(6):  # (the LRU holds a handful)
        cs.solve(max_iter=600 + k)
    assert K.cg_sessions_live() <= live0 + 4
    # ensure_q() changes a root-form-only cache: its sessions go, the next solve is correct and starts a new one
    cs.pre = cs.build(need_q=False)
    gc.collect()
    assert cs.pre.Q is None and K.cg_sessions_live() == live0
    got = cs.solve()
    same(got, general(cs))
    assert torch.equal(got[0].x, ref[0].x)
    assert K.cg_sessions_live() == live0 + 1
    cs.pre.ensure_q()
    assert cs.pre.Q is not None and K.cg_sessions_live() == live0
    same(cs.solve(), general(cs))
    assert K.cg_sessions_live() == live0 + 1
    # a preconditioner rebuilt for the same operator (a new generation)
    old_gen = cs.pre.generation
    cs.pre = cs.build()
    gc.collect()
    assert cs.pre.generation != old_gen and K.cg_sessions_live() == live0
    same(cs.solve(), ref)
    assert K.cg_sessions_live() == live0 + 1
    # the cache deleted
    cs.pre = None
    gc.collect()
    assert K.cg_sessions_live() == live0


def entry_points_that_launched(fn):
    """Which entry points launched k_cg_rspace3 and saw its ticket while fn() ran: {name: count} from the library's host
    intervals ("cg_session": lo_cg_session_solve_f32 returned LO_OK; "cg_solve": lo_cg_solve_f32 did)."""
    K._hip.prof_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
        rep = K._hip.prof_report()
    finally:
        K._hip.prof_enable(False)
    return out, {n[len("host:"):-len("_entry_to_launch")]: v[0] for n, v in rep.items() if n.endswith("_entry_to_launch")}


def test_a_fresh_descriptor_on_every_solve_reuses_the_session():
    # the operator classes lower themselves anew for every solve: new descriptor, new views of the same storage
    cs = Case(9251, 5, 1500, 16)
    live0 = K.cg_sessions_live()
    ref = general(cs)
    A0, d = cs.desc.A0, cs.desc.d

    def solves():
        out = []
        for i in range(6):
            cs.desc = K.lowrank_diag_descriptor(A0.view(A0.shape), d.view(d.shape))
            assert cs.desc.A0 is not A0 and cs.desc.A0.data_ptr() == A0.data_ptr()
            out.append(cs.solve())
            assert K.cg_sessions_live() == live0 + 1, i
        return out

    out, launched = entry_points_that_launched(solves)
    assert launched == {"cg_session": 6}, launched
    for got in out:
        same(got, ref)


def test_two_operators_alternately_keep_two_sessions():
    live0 = K.cg_sessions_live()
    a, b = Case(9301, 3, 256, 8), Case(9302, 5, 1500, 16)
    refs = [[general(c, i) for i in range(2)] for c in (a, b)]
    for rnd in range(3):
        for j, c in enumerate((a, b)):
            same(c.solve(rnd % 2), refs[j][rnd % 2])
        assert K.cg_sessions_live() == live0 + 2
    del a, b, c
    gc.collect()
    assert K.cg_sessions_live() == live0


def test_switches_flipped_while_a_session_is_alive():
    cs = Case(9401, 70, 2500, 32)
    cs.pre.ensure_q()  # (for the streaming engine below; a cache without Q would build it then, and drop its session)
    live0 = K.cg_sessions_live()
    ref = cs.solve()
    assert ref[1]["rspace"] == "resident" and ref[1]["rspace_diag"] and K.cg_sessions_live() == live0 + 1
    same(ref, general(cs))
    with env("LO_OC_NO_RSPACE"):
        got = cs.solve()
        assert got[1]["rspace"] == "none", got[1]
        same(got, general(cs))
    same(cs.solve(), ref)
    with env("LO_RS_NO_DIAG"):
        got = cs.solve()
        assert got[1]["rspace"] == "resident" and not got[1]["rspace_diag"], got[1]
        same(got, general(cs))
    same(cs.solve(), ref)
    K.set_onchip_cg(False)
    got = cs.solve()
    assert got[1]["rspace"] == "none" and not got[1]["resident"], got[1]
    same(got, general(cs))
    K.set_onchip_cg(True)
    same(cs.solve(), ref)
    assert K.cg_sessions_live() == live0 + 1  # (the one session served throughout)


def test_injected_timeout_is_counted_once_and_cools_down():
    cs = Case(9501, 5, 1500, 16)
    cs.pre.ensure_q()  # (the streaming engine applies the Q form)
    ref = cs.solve()
    K.set_onchip_cg(False)
    streamed = cs.solve()  # the streaming engine from iteration 0: what a redo after a lost hand-off runs
    K.set_onchip_cg(True)
    assert not streamed[1]["resident"]
    s0, h0 = K.resident_status(), K.resident_handoff_debug()
    K.inject_resident_timeouts(1)
    hit, e = cs.solve()  # the session's launch starts with its error word set: the general path redoes the solve
    s1 = K.resident_status()
    assert not e["resident"] and e["streaming_iterations"] >= 11, e
    assert s1["timeouts"] == s0["timeouts"] + 1 and s1["cooldown"] == s0["backoff"], (s0, s1)
    same((hit, e), streamed)
    for _ in range(s1["cooldown"] - 1):  # the cool-down, as long as without sessions
        assert not cs.solve()[1]["resident"]
    back = cs.solve()  # re-armed: k_cg_rspace3 again, behind ONE clearing of the hand-off block
    h1, s2 = K.resident_handoff_debug(), K.resident_status()
    same(back, ref)
    assert h1["clears"] == h0["clears"] + 1 and h1["launches"] == h0["launches"] + 2
    assert s2["timeouts"] == s0["timeouts"] + 1 and s2["cooldown"] == 0
    same(cs.solve(), ref)
    assert K.resident_handoff_debug()["clears"] == h1["clears"]


def test_right_hand_side_inside_the_span_of_the_root_runs_the_dense_form():
    cs = Case(9601, 5, 1500, 16)
    w = np.random.default_rng(9602).standard_normal((5, 16, 1)).astype(np.float32)
    rhs = dev(cs.C @ w)
    got = cs.solve(rhs=rhs)
    assert got[1]["rspace"] == "resident" and not got[1]["rspace_diag"], got[1]
    with env("LO_CG_NO_SESSION"):
        same(got, cs.solve(rhs=rhs))
    same(cs.solve(), general(cs))


def test_batch_with_an_all_zero_member():
    cs = Case(9701, 5, 1500, 16)
    rhs = cs.rhs[0].clone()
    rhs[2] = 0
    got = cs.solve(rhs=rhs)
    with env("LO_CG_NO_SESSION"):
        same(got, cs.solve(rhs=rhs))
    assert torch.count_nonzero(got[0].x[2]) == 0 and torch.isfinite(got[0].x).all()


def test_a_lean_miss_goes_to_the_general_path_and_is_remembered():
    # tolerance 1e-30: no fp32 residual norm gets there in the 11 iterations of the floor -- the result-only pass misses
    runs = {}
    for mode in ("session", "general"):
        K.set_onchip_cg(True)  # (forgets the misses of the other mode)
        cs = Case(9801, 5, 1500, 16)
        cs.pre.ensure_q()  # (the streaming engine continues past the floor)
        with env("LO_CG_NO_SESSION", mode == "general"):
            runs[mode] = [cs.solve(tolerance=1e-30, max_iter=14) for _ in range(2)]
    for a, b in zip(runs["session"], runs["general"]):
        same(a, b)
    first, second = runs["session"]
    assert first[0].iterations > 11 and not first[0].tolerance_reached
    assert not second[1]["lean"], second[1]  # (lean_miss_find: the state-writing pass right away)


def under_capture(cs):
    """One headline solve inside a torch.cuda.graph capture: what came back (or what was raised), and what it did to the
    gate, the hand-off block and the sessions."""
    s0, h0, live0 = K.resident_status(), K.resident_handoff_debug(), K.cg_sessions_live()
    graph = torch.cuda.CUDAGraph()

    def run():
        try:
            with torch.cuda.graph(graph):
                res = cs.solve()
            return ("returned", fields(res[0]), res[1])
        except Exception as e:  # noqa: BLE001 -- the outcome IS the exception
            return ("raised", type(e).__name__, str(e).splitlines()[0] if str(e) else "")

    outcome, launched = entry_points_that_launched(run)
    s1, h1 = K.resident_status(), K.resident_handoff_debug()
    effects = ({k: s1[k] - s0[k] for k in s0}, h1["launches"] - h0["launches"], h1["clears"] - h0["clears"],
               K.cg_sessions_live() - live0)
    return outcome, effects, launched


def test_under_stream_capture_the_session_refuses_and_the_call_behaves_as_the_general_path():
    """Measured on the parent first: a headline solve inside a capture takes the cleared-workspace path (host-assigned
    hand-off tags must not be baked into a graph), its wait for the ticket ends in a stream synchronisation the capture
    forbids, the capture is invalidated and the call raises -- and the process's HIP state stays broken for the solves
    behind it.  So each path gets a process of its own here (that is what this test is about): the session path must end
    the same way with the same side effects, and must not have launched anything itself."""
    import json
    import subprocess
    import sys

    outs = {}
    for mode in ("general", "session"):
        e = dict(os.environ)
        e.pop("LO_CG_NO_SESSION", None)
        if mode == "general":
            e["LO_CG_NO_SESSION"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    want, got = outs["general"], outs["session"]
    assert want["outcome"][0] == "raised" and "capture" in want["outcome"][2], want  # (the parent's behaviour)
    assert got["outcome"] == want["outcome"], (got, want)
    # no time-out noted, no cool-down, nothing launched on or cleared from the library's hand-off block
    assert want["effects"][0] == {k: 0 for k in want["effects"][0]} and want["effects"][1:3] == [0, 0], want
    assert got["effects"][:3] == want["effects"][:3], (got, want)
    assert got["sessions"] == 1 and want["sessions"] == 0  # (the session stays, unused; the general path makes none)
    assert "cg_session" not in got["launched"], got
    assert got["before"] == {"cg_session": 1} and want["before"] == {"cg_solve": 1}, (got, want)


if __name__ == "__main__":  # the child process of the capture test: one path, chosen by LO_CG_NO_SESSION
    import json

    cs = Case(9901, 5, 1500, 16)
    cs.solve()
    _, before = entry_points_that_launched(cs.solve)  # (which entry point serves a solve outside the capture)
    live = K.cg_sessions_live()
    outcome, effects, launched = under_capture(cs)
    print(json.dumps({"outcome": outcome, "effects": effects, "launched": launched, "before": before, "sessions": live}))
