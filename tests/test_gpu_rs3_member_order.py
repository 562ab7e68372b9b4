"""k_cg_rspace3 walks the members of a batch in either direction (csrc/lo_rspace3.hip): groups draw LOGICAL
indices as ever and address the PHYSICAL member m = flip ? B - 1 - b : b, so that a solve on the operator of the previous
solve starts with the members that one read last (memory-side cache).  The order enters no result.

Every member of every case is its own random system (cases.lowrank_diag): taking a logical index where the physical one
belongs -- operator, right-hand side, diagonal, matrices, x, records, close granule, the deferred norm, the next member's
requests -- changes x or the mean residual.  Shapes, the smallest that reach each branch on a 256-CU device (512 / GW
groups), each also on a quarter of the groups (LO_OC_RESERVE_CUS=192: several rounds):

  (1, 8192, 32)    one member
  (3, 256, 8)      fewer members than groups: most groups never enter the loop and close behind it
  (70, 1000, 16)   N no multiple of 256: the row clamp, rows shared between two waves' loads
  (37, 2304, 32)   three workgroups of a group of four hold rows, the last one partly
  (150, 8192, 32)  the headline instantiation <32, 8>; with the reserve >= 9 rounds: the deferred last norm (late_v) and
                   the x pass' requests for the next member, reversed
  (130, 4096, 8)   a constant diagonal: 1 / d per member, not per row

For each: forced forward, forced reverse and three automatic solves return the same x and the same mean residual bit for
bit, the library reports forward, reverse, forward, reverse, forward, and x meets the fp64 Woodbury solution.  Then the
rule that decides who flips, and the peer buffers under reversal.  Without a GPU: the binding of the debug export.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import cases
import test_gpu_early_ticket as et

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(1, 8192, 32), (3, 256, 8), (70, 1000, 16), (37, 2304, 32), (150, 8192, 32), (130, 4096, 8)]
CONST_DIAG = (130, 4096, 8)
PEER_SHAPE = (40, 1024, 16)

_form_on_second_use = et._form_on_second_use  # (autouse: the diagonal form on second use, switches restored)


class ConstDiagCase(et.Case):
    """et.Case with one diagonal value per member (LO_DIAG_CONST: the kernel reads 1 / d of the member, not of a row)."""

    def __init__(self, seed, B, N, R):
        self.shape = (B, N, R)
        C, _, rhs = cases.lowrank_diag(seed, B, N, R, 1)
        sig = (0.5 + np.random.default_rng(seed + 2).random(B)).astype(np.float32)
        self.C, self.d = C, np.repeat(sig[:, None], N, 1)  # (self.d: the full diagonal, for the closed form)
        self.desc = K.lowrank_diag_descriptor(et.dev(C), et.dev(sig), const_diag=True)
        L, perm = K.pivoted_cholesky(self.desc, 15)
        self.pre = K.precond_build(L, et.dev(sig), constant_diag=True, root=self.desc.A0, perm=perm)
        self.rhs_host = [rhs]
        self.rhs = [et.dev(rhs)]
        self.solve(self.rhs[0])
        self.solve(self.rhs[0])
        assert torch.is_tensor(self.pre.RSD)
        self.refs = [self.solve_owned(self.rhs[0])[0]]
        torch.cuda.synchronize()


_cases = {}


def case(shape):
    if shape not in _cases:
        seed = 9500 + (SHAPES + [PEER_SHAPE]).index(shape)
        _cases[shape] = (ConstDiagCase if shape == CONST_DIAG else et.Case)(seed, *shape)
    return _cases[shape]


def solve_dir(cs, mode=None):
    """One solve on the library's buffer, optionally under a forced order: (result, direction the library reports)."""
    if mode is not None:
        K.resident_order_debug(mode)
    n0 = K.resident_order_debug()["reversed"]
    res, _ = cs.solve_owned(cs.rhs[0])
    st = K.resident_order_debug()
    assert st["reversed"] - n0 == (1 if st["last"] == "reverse" else 0)
    return res, st["last"]


@gpu
@pytest.mark.parametrize("reserve", [None, "192"], ids=["whole_device", "quarter_of_the_groups"])
@pytest.mark.parametrize("shape", SHAPES)
def test_results_do_not_depend_on_the_order(shape, reserve, monkeypatch):
    cs = case(shape)
    if reserve:
        monkeypatch.setenv("LO_OC_RESERVE_CUS", reserve)
    try:
        runs = [solve_dir(cs, 1), solve_dir(cs, 2), solve_dir(cs, 0), solve_dir(cs), solve_dir(cs)]
    finally:
        K.resident_order_debug(0)
    torch.cuda.synchronize()
    # automatic behind a forced reverse launch on the same operator: forward, then alternating
    assert [d for _, d in runs] == ["forward", "reverse", "forward", "reverse", "forward"]
    first = runs[0][0]
    for i, (res, d) in enumerate(runs[1:], 1):
        assert torch.equal(res.x, first.x), f"solve {i} ({d}): x depends on the order"
        assert res.mean_residual == first.mean_residual, (i, d, res.mean_residual, first.mean_residual)
        assert res.iterations == first.iterations and res.tolerance_reached == first.tolerance_reached
        assert not res.nan_detected
    # ... and on neither the grid nor the solves of the set-up
    assert torch.equal(first.x, cs.refs[0].x) and first.mean_residual == cs.refs[0].mean_residual
    ex = et.woodbury(cs.C, cs.d, cs.rhs_host[0])
    err = float(((runs[1][0].x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
    print(f"{shape} reserve={reserve}: reverse solve against fp64 Woodbury {err:.3e}")
    assert err < 1e-4, err  # (the bound of tests/test_gpu_rs3_member_path.py)


@gpu
def test_the_flip_rule():
    """An owned launch on the operator (C, B, N, RC) of the previous owned launch runs the other way round when that one
    was confirmed clean; every other launch runs forward.  A forced clear of the hand-off buffer does NOT reset the
    order (clearing says nothing about what the cache holds): the solve behind it still alternates."""
    a, b = case((70, 1000, 16)), case((3, 256, 8))
    K.resident_order_debug(0)
    try:
        solve_dir(b)
        assert solve_dir(a)[1] == "forward"   # another operator
        assert solve_dir(a)[1] == "reverse"
        assert solve_dir(b)[1] == "forward"   # another operator, although the last launch ran in reverse
        assert solve_dir(b)[1] == "reverse"
        assert solve_dir(b)[1] == "forward"
        K.resident_handoff_debug(force_clear=True)
        h0 = K.resident_handoff_debug()
        res, d = solve_dir(b)
        assert K.resident_handoff_debug()["clears"] == h0["clears"] + 1
        assert d == "reverse", "a forced clear must not reset the order"
        assert torch.equal(res.x, b.refs[0].x) and res.mean_residual == b.refs[0].mean_residual
        # an injected hand-off time-out: that launch is never confirmed, so the next owned launch runs forward -- by
        # alternation alone it would run in reverse (the injected launch itself, behind a clean reverse one, ran forward)
        s0 = K.resident_status()
        n0 = K.resident_order_debug()["reversed"]
        K.inject_resident_timeouts(1)
        hit = b.solve(b.rhs[0])
        s1 = K.resident_status()
        assert s1["timeouts"] == s0["timeouts"] + 1 and s1["cooldown"] > 0
        st = K.resident_order_debug()
        assert st["last"] == "forward" and st["reversed"] == n0
        assert hit.iterations == b.refs[0].iterations
        for _ in range(s1["cooldown"] - 1):  # the cool-down: fall-back engine, no launch of k_cg_rspace3
            b.solve(b.rhs[0])
        assert K.resident_order_debug()["reversed"] == n0
        res, d = solve_dir(b)
        assert d == "forward", "the launch behind an unconfirmed one must run forward"
        assert torch.equal(res.x, b.refs[0].x) and res.mean_residual == b.refs[0].mean_residual
        assert solve_dir(b)[1] == "reverse"
    finally:
        K.resident_order_debug(0)
        K.inject_resident_timeouts(0)


@gpu
def test_peer_buffer_holds_x_under_reversal():
    cs = case(PEER_SHAPE)
    B, N, _ = PEER_SHAPE
    peer = torch.zeros(2 * B, N, device="cuda")  # this rank's members at [B, 2 B) of the peer's buffer
    try:
        K.peer_gather_set([peer], B)
        res, d = solve_dir(cs, 2)
        torch.cuda.synchronize()
        assert d == "reverse"
        assert torch.equal(res.x, cs.refs[0].x) and res.mean_residual == cs.refs[0].mean_residual
        assert torch.equal(peer[B:], res.x[..., 0]), "the peer buffer does not hold x"
        assert float(peer[:B].abs().max()) == 0.0, "the peer's other slice was written"
    finally:
        K.peer_gather_set(())
        K.resident_order_debug(0)


# ---- without a GPU ----
def test_binding_of_the_order_export():
    assert _hip.ABI_VERSION >= 32
    name = "lo_resident_order_debug"
    assert name in _hip._PROTOTYPES and name in _hip.EXPORTS
    restype, argtypes = _hip._PROTOTYPES[name]
    assert restype is ctypes.c_int and len(argtypes) == 2
    assert argtypes[0] is ctypes.c_int32 and argtypes[1] is ctypes.POINTER(ctypes.c_uint32)
    assert hasattr(ctypes.CDLL(_hip.lib_path()), name), "liblo_amd.so does not export " + name
    assert _hip.load().lo_abi_version() == _hip.ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lo_amd.h")).read()
    assert "int lo_resident_order_debug(int32_t mode, uint32_t* out);" in hdr
    # (the hand-off call keeps its four words)
    assert len(_hip._PROTOTYPES["lo_resident_handoff_debug"][1]) == 4
