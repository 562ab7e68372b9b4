"""The native entry of the session solve (csrc/lo_pyfast.cpp, `kernels.cg_fast_entry`) on the device: the
same launches through another binding, so everything is compared bit for bit -- the native entry forced against the
ctypes session path (the entry forbidden) and against the general path (LO_CG_NO_SESSION).  Shapes, cases and helpers are
those of tests/test_gpu_cg_session.py: (3, 256, 8) one workgroup per group, (5, 1500, 16) two, (70, 2500, 32) more members
than resident groups.
"""
import gc
import os
import sys
import threading
from dataclasses import replace

if __name__ == "__main__":  # (run as the capture test's child: what conftest.py puts on the path for the suite)
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), os.path.join(_here, "golden")]

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from linear_operator_amd import kernels as K  # noqa: E402
from test_gpu_cg_session import (SHAPES, Case, _clean_gate, dev, entry_points_that_launched, env, fields,  # noqa: E402,F401
                                 same, under_capture)


class Counting:
    """Stands where kernels keeps the extension module: counts the native calls, keeps their return codes, and runs a
    hook in front of the call (the caller is then inside the session: its `busy` lock is held)."""

    def __init__(self, mod):
        self.mod, self.rcs, self.before, self.around = mod, [], None, None

    def session_solve(self, *args):
        if self.before is not None:
            self.before()
        if self.around is not None:
            return self.around(lambda: self._call(*args))
        return self._call(*args)

    def _call(self, *args):
        out = self.mod.session_solve(*args)
        self.rcs.append(out[0])
        return out


@pytest.fixture
def native():
    """The native entry forced, with the counter in place; automatic again afterwards."""
    assert K.cg_fast_entry(True) == "native"
    K._fast_module = cnt = Counting(K._fast_module)
    yield cnt
    K.cg_fast_entry(None)


def forbid(cnt):
    assert K.cg_fast_entry(False) == "ctypes"
    K._fast_module = cnt  # (stays in place: nothing may reach it while the entry is forbidden)


def force(cnt):
    assert K.cg_fast_entry(True) == "native"
    K._fast_module = cnt


def rhs_forms(cs, i):
    """Right-hand side i of the case as [B, N, 1] contiguous, batch-shaped ([2, B/2, N, 1]; [1, B, N, 1] for an odd B) and
    as a non-contiguous [B, N, 1] (every other column of a [B, N, 2] buffer)."""
    r = cs.rhs[i]
    B, N, _ = r.shape
    wide = torch.stack([r[..., 0], -r[..., 0]], dim=-1)
    strided = wide[..., :1]
    assert not strided.is_contiguous() and torch.equal(strided, r)
    return {"contiguous": r, "batch": r.reshape((2, B // 2, N, 1) if B % 2 == 0 else (1, B, N, 1)), "strided": strided}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_equality_of_the_three_paths(shape, native):
    cs = Case(9150 + shape[0], *shape)
    runs = {}
    for mode in ("native", "ctypes", "general"):
        (force if mode == "native" else forbid)(native)
        n0, uses0, out = len(native.rcs), cs.pre.rs_uses, []
        with env("LO_CG_NO_SESSION", mode == "general"):
            for form in ("contiguous", "batch", "strided"):
                for i in range(3):  # three solves in a row, three right-hand sides
                    rhs = rhs_forms(cs, i)[form]
                    res, ex = cs.solve(rhs=rhs)
                    assert res.x.shape == rhs.shape and res.x.is_contiguous()
                    out.append((res, ex))
        runs[mode] = out
        assert cs.pre.rs_uses - uses0 == 9, mode
        assert native.rcs[n0:] == ([0] * 9 if mode == "native" else []), mode
    for k in range(9):
        for other in ("ctypes", "general"):
            same(runs["native"][k], runs[other][k])
        assert runs["native"][k][1]["rspace"] == "resident" and runs["native"][k][1]["rspace_diag"]
    assert torch.equal(runs["native"][0][0].x.reshape(-1), runs["native"][3][0].x.reshape(-1))  # (one rhs, two layouts)
    assert not torch.equal(runs["native"][0][0].x, runs["native"][1][0].x)


def same_bits(a, b):
    """`same` for results that may hold NaN (which no `torch.equal` finds equal): x as bit patterns."""
    (ra, ea), (rb, eb) = a, b
    same((replace(ra, x=ra.x.view(torch.int32)), ea), (replace(rb, x=rb.x.view(torch.int32)), eb))


def step(cs, s0, uses0, **kw):
    """One solve with everything the two bindings must agree on: the result (or what was raised), what ran, the gate's
    counters since s0, and the solves the cache counts."""
    try:
        got = cs.solve(**kw)
    except Exception as e:  # noqa: BLE001 -- the outcome is compared
        got = ("raised", type(e).__name__, str(e))
    s1 = K.resident_status()
    return got, {k: s1[k] - s0[k] for k in s0}, cs.pre.rs_uses - uses0


def on_both_bindings(native, seed, shape, scenario):
    """scenario(cs, record) on a fresh case per binding; the records must agree.  Returns the native entry's records and its
    return codes."""
    recs = {}
    for mode in ("native", "ctypes"):
        K.inject_resident_timeouts(0)
        K.set_onchip_cg(True)
        (force if mode == "native" else forbid)(native)
        n0 = len(native.rcs)
        cs = Case(seed, *shape)
        cs.pre.ensure_q()  # (the streaming engine applies the Q form)
        s0, uses0, out = K.resident_status(), cs.pre.rs_uses, []
        scenario(cs, lambda **kw: out.append(step(cs, s0, uses0, **kw)) or out[-1])
        recs[mode] = out
        rcs = native.rcs[n0:]
        assert mode == "native" or not rcs
        if mode == "native":
            native_rcs = rcs
        del cs
        gc.collect()
    assert len(recs["native"]) == len(recs["ctypes"])
    for (ga, sa, ua), (gb, sb, ub) in zip(recs["native"], recs["ctypes"]):
        if ga[0] == "raised" or gb[0] == "raised":
            assert ga == gb
        else:
            same_bits(ga, gb)
        assert sa == sb and ua == ub, (sa, sb, ua, ub)
    return recs["native"], native_rcs


def test_injected_timeout_through_the_native_entry(native):
    def scenario(cs, solve):
        solve()
        K.inject_resident_timeouts(1)
        hit = solve()
        for _ in range(hit[1]["cooldown"] - 1):
            solve()
        solve()  # re-armed
        solve()

    recs, rcs = on_both_bindings(native, 9511, (5, 1500, 16), scenario)
    ref, hit, back, last = recs[0], recs[1], recs[-2], recs[-1]
    assert hit[1]["timeouts"] == 1 and hit[1]["cooldown"] > 0 and not hit[0][1]["resident"], hit
    assert all(not r[0][1]["resident"] for r in recs[2:-2])  # the cool-down runs ...
    same(back[0], ref[0])  # ... and the resident path comes back
    same(last[0], ref[0])
    assert last[1]["timeouts"] == 1 and last[1]["cooldown"] == 0  # counted once
    # the native entry handed over exactly the solves that did not stay on the session (LO_ERR_UNSUPPORTED, no exception)
    assert rcs[0] == 0 and rcs[1] == K._hip.LO_ERR_UNSUPPORTED and rcs[-1] == 0, rcs
    assert set(rcs) <= {0, K._hip.LO_ERR_UNSUPPORTED} and len(rcs) == len(recs), rcs
    assert ref[2] == 1 and last[2] == 3  # (rs_uses: the three resident solves)


def test_switch_flipped_while_the_session_lives(native):
    def scenario(cs, solve):
        solve()
        with env("LO_OC_NO_RSPACE"):
            solve()
        solve()
        with env("LO_RS_NO_DIAG"):
            solve()
        solve()

    recs, rcs = on_both_bindings(native, 9411, (70, 2500, 32), scenario)
    assert rcs == [0, K._hip.LO_ERR_UNSUPPORTED, 0, K._hip.LO_ERR_UNSUPPORTED, 0], rcs
    assert recs[1][0][1]["rspace"] == "none" and not recs[3][0][1]["rspace_diag"]
    same(recs[2][0], recs[0][0])
    same(recs[4][0], recs[0][0])


def test_delicate_right_hand_sides_through_the_native_entry(native):
    def scenario(cs, solve):
        w = np.random.default_rng(9612).standard_normal((5, 16, 1)).astype(np.float32)
        solve(rhs=dev(cs.C @ w))  # inside span(C)
        zero = cs.rhs[0].clone()
        zero[2] = 0
        solve(rhs=zero)  # an all-zero member
        nan = cs.rhs[1].clone()
        nan[1, 7, 0] = float("nan")
        solve(rhs=nan)
        solve()

    recs, rcs = on_both_bindings(native, 9611, (5, 1500, 16), scenario)
    span, zero, nan, plain = recs
    assert span[0][1]["rspace"] == "resident" and not span[0][1]["rspace_diag"], span[0][1]
    assert torch.count_nonzero(zero[0][0].x[2]) == 0 and torch.isfinite(zero[0][0].x).all()
    assert nan[0][0] == "raised" or nan[0][0].nan_detected or not torch.isfinite(nan[0][0].x).all()
    assert rcs[0] == K._hip.LO_ERR_UNSUPPORTED and rcs[-1] == 0, rcs  # span(C): the general path's dense form
    assert plain[0][1]["rspace_diag"]


def test_busy_session_second_thread_takes_the_general_path(native):
    cs = Case(9421, 70, 2500, 32)
    ref = cs.solve()
    ref2 = cs.solve(1)
    inside, done, other = threading.Event(), threading.Event(), {}

    def second():
        inside.wait(30)
        try:
            other["out"], other["launched"] = entry_points_that_launched(lambda: cs.solve(1))
        finally:
            done.set()

    def before():  # (in the first thread, inside its solve: the session is busy until the hook returns)
        native.before = None
        inside.set()
        assert done.wait(60)

    t = threading.Thread(target=second)
    t.start()
    native.before = before
    n0 = len(native.rcs)
    first = cs.solve()
    t.join()
    assert other["launched"] == {"cg_solve": 1}, other["launched"]  # the general entry point, not the session's
    assert native.rcs[n0:] == [0]
    assert torch.equal(other["out"][0].x, ref2[0].x) and fields(other["out"][0]) == fields(ref2[0])
    same(first, ref)


def test_the_gil_is_released_during_the_native_call(native):
    cs = Case(9431, 70, 2500, 32)
    cs.solve()
    count, stop, progress = [0], threading.Event(), []

    def counter():
        while not stop.is_set():
            count[0] += 1

    def around(call):  # (only the native call lies between the two reads)
        n0 = count[0]
        out = call()
        progress.append(count[0] - n0)
        return out

    old = sys.getswitchinterval()
    sys.setswitchinterval(1e-4)
    t = threading.Thread(target=counter)
    t.start()
    try:
        native.around = around
        for i in range(10):
            cs.solve(i % 4)
    finally:
        native.around = None
        stop.set()
        t.join()
        sys.setswitchinterval(old)
    print("counts during the ten native calls:", progress)
    assert len(progress) == 10 and sum(p > 0 for p in progress) >= 5 and sum(progress) >= 10, progress


def test_sessions_end_with_their_caches(native):
    live0 = K.cg_sessions_live()
    cases = [Case(9441 + k, *SHAPES[k]) for k in range(2)]
    for cs in cases:
        cs.solve()
        cs.solve(1)
    assert K.cg_sessions_live() == live0 + 2 and native.rcs[-4:] == [0] * 4
    cases[0].pre.drop_sessions()
    assert K.cg_sessions_live() == live0 + 1
    del cases, cs
    gc.collect()
    assert K.cg_sessions_live() == live0


def test_memo_in_front_of_the_lru(native):
    live0 = K.cg_sessions_live()
    cs = Case(9451, 5, 1500, 16)
    with env("LO_CG_NO_SESSION"):
        ref = cs.solve()
    pre = cs.pre
    assert pre._memo is None
    same(cs.solve(), ref)
    ent = pre._memo[0]
    assert pre._memo[1] is cs.desc and list(pre._sessions.values()) == [ent]
    same(cs.solve(), ref)
    assert pre._memo[0] is ent and K.cg_sessions_live() == live0 + 1
    # a descriptor rebuilt over the same storage: found by the key, remembered in its turn
    A0, d = cs.desc.A0, cs.desc.d
    cs.desc = K.lowrank_diag_descriptor(A0.view(A0.shape), d.view(d.shape))
    same(cs.solve(), ref)
    assert pre._memo[0] is ent and pre._memo[1] is cs.desc and K.cg_sessions_live() == live0 + 1
    # another tolerance: a miss, the second session; back again: the first one, through the LRU
    with env("LO_CG_NO_SESSION"):
        ref3 = cs.solve(tolerance=1e-3)
    same(cs.solve(tolerance=1e-3), ref3)
    assert pre._memo[0] is not ent and K.cg_sessions_live() == live0 + 2 and len(pre._sessions) == 2
    same(cs.solve(), ref)
    assert pre._memo[0] is ent and list(pre._sessions.values())[-1] is ent
    # what changes the cache drops the memo with the sessions
    pre.drop_sessions()
    assert pre._memo is None and K.cg_sessions_live() == live0
    same(cs.solve(), ref)
    assert pre._memo is not None
    rsd, pre.RSD = pre.RSD, None  # (a cache that is about to get its diagonal form)
    pre.ensure_eigform()
    assert pre._memo is None and K.cg_sessions_live() == live0 and torch.equal(pre.RSD, rsd)
    same(cs.solve(), ref)
    cs.pre = pre = cs.build(need_q=False)  # (a root-form-only cache: its plan names another streaming engine)
    gc.collect()
    with env("LO_CG_NO_SESSION"):
        ref_root = cs.solve()
    got = cs.solve()
    same(got, ref_root)
    assert torch.equal(got[0].x, ref[0].x) and pre._memo is not None and pre.Q is None
    pre.ensure_q()
    assert pre._memo is None and pre.Q is not None and K.cg_sessions_live() == live0
    with env("LO_CG_NO_SESSION"):
        ref_q = cs.solve()
    got = cs.solve()
    same(got, ref_q)
    assert torch.equal(got[0].x, ref[0].x) and pre._memo is not None
    assert native.rcs == [0] * 9  # (every session solve above, and each through the native entry)


def test_under_stream_capture_the_native_entry_behaves_as_the_ctypes_session_path():
    """As tests/test_gpu_cg_session.py's capture test: a process per binding (a capture that was invalidated leaves the
    process's HIP state broken), the same outcome and side effects, and nothing launched by the session entry."""
    import json
    import subprocess

    outs = {}
    for mode in ("ctypes", "native"):
        e = dict(os.environ)
        e.pop("LO_CG_NO_SESSION", None)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], env=e, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (mode, r.stdout[-2000:], r.stderr[-2000:])
        outs[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    want, got = outs["ctypes"], outs["native"]
    assert want["entry"] == "ctypes" and got["entry"] == "native"
    assert want["outcome"][0] == "raised" and "capture" in want["outcome"][2], want
    assert got["outcome"] == want["outcome"], (got, want)
    assert got["effects"] == want["effects"], (got, want)
    assert got["sessions"] == want["sessions"] == 1
    assert "cg_session" not in got["launched"] and got["launched"] == want["launched"], (got, want)
    assert got["before"] == want["before"] == {"cg_session": 1}, (got, want)
    assert got["native_rcs"][:2] == [0, 0] and got["native_rcs"][2:] == [K._hip.LO_ERR_UNSUPPORTED], got
    assert want["native_rcs"] == []


if __name__ == "__main__":  # the child process of the capture test: one binding, named on the command line
    import json

    mode = sys.argv[1]
    entry = K.cg_fast_entry(mode == "native")
    K._fast_module = cnt = Counting(K._fast_module)
    cs = Case(9901, 5, 1500, 16)
    cs.solve()
    _, before = entry_points_that_launched(cs.solve)
    live = K.cg_sessions_live()
    outcome, effects, launched = under_capture(cs)
    print(json.dumps({"entry": entry, "outcome": outcome, "effects": effects, "launched": launched, "before": before,
                      "sessions": live, "native_rcs": cnt.rcs}))
