"""The ordered start of k_cg_rspace3 (csrc/lo_rs3_start.h, csrc/lo_rspace3.hip): in a launch of six rounds
or more the workgroups of a group wait, before they request anything, a number of clock ticks that depends on the group
alone -- (the group's index inside its dispatch wave) x delta -- where no group of the layout waits more than three
steps.  The wait reads the clock and nothing else: it enters no result, a group without a member skips it and still
closes, and it ends at the cap whatever it is given.

Shapes (N, R) with the group widths the library chooses for them -- (256, 8) and (1000, 16): one workgroup per member;
(2048, 8): two; (8192, 32): eight, the headline instantiation -- each on the whole device and on a quarter of the groups
(LO_OC_RESERVE_CUS=192), and for each the batch sizes that reach every branch of the start, chosen against the number of
groups G of the device under test:

  B = G / 4 - 1   fewer members than groups: the groups without a member skip the wait and close behind the loop
  B = G           a single round
  B = G + 1       two rounds, one group draws a second member
  B = 3 G + 5     four rounds, the last one ragged (automatic: still no wait)
  B = 5 G + 3     six rounds (the smallest and the headline shape only): automatic waits where the layout allows it --
                  8 groups per XCD, the headline shape on the whole device -- and nowhere else

For each: the start forced off, forced on with the committed delay (walking forward and in reverse), forced on with the
cap as delta (forward and in reverse), and automatic return the same x and the same mean residual bit for bit; the
library reports the mode, the delta and the groups of each launch; x meets the fp64 Woodbury solution within the bound
of tests/test_gpu_rs3_member_order.py.  Then an injected hand-off time-out under a forced start.  Without a GPU: the
delay rule against a table, the cap, the binding.
"""
import ctypes
import os

import pytest
import torch

import test_gpu_early_ticket as et

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402

gpu = pytest.mark.gpu

CAP = 800                           # ticks of the 100 MHz clock: 8 us
DELTA, MIN_ROUNDS, MAX_STEPS = 200, 6, 3       # the committed delta; automatic from six rounds on, up to three steps
SHAPES = [(256, 8, 1), (1000, 16, 1), (2048, 8, 2), (8192, 32, 8)]  # (N, R, workgroups per member)
RULES = {"fewer_than_groups": lambda g: g // 4 - 1, "one_round": lambda g: g, "one_more": lambda g: g + 1,
         "four_rounds": lambda g: 3 * g + 5, "six_rounds": lambda g: 5 * g + 3}
# (six rounds at the smallest and at the headline shape only: the suite stays quick)
SHAPE_RULES = [(s, r) for s in SHAPES for r in RULES if r != "six_rounds" or s in (SHAPES[0], SHAPES[3])]
AUTO, OFF, ON, GIVEN = 0, 1, 2, 3

_form_on_second_use = et._form_on_second_use  # (autouse: the diagonal form on second use, switches restored)


def ngroups_of(gw, reserve):
    """Groups of a k_cg_rspace3 launch: two workgroups per CU (in 32s), 8 XCDs, whole groups per XCD."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if reserve:
        cus = max(64, cus - int(reserve))
    return (2 * (cus // 32 * 32) // 8 // gw) * 8


_cases = {}


def case(N, R, B):
    key = (B, N, R)
    if key not in _cases:
        _cases[key] = et.Case(9600 + (31 * N + 7 * R + B) % 389, B, N, R)
    return _cases[key]


def solve_start(cs, mode, delta=0, order=0):
    """One solve on the library's buffer under (start mode, delta, walk order): (result, what the launch used)."""
    K.resident_start_debug(mode, delta)
    K.resident_order_debug(order)
    w0 = K.resident_start_debug()["waited"]
    res, _ = cs.solve_owned(cs.rhs[0])
    st = K.resident_start_debug()
    assert st["mode"] == mode
    assert st["waited"] - w0 == (1 if st["delta"] else 0)
    return res, st


@gpu
@pytest.mark.parametrize("reserve", [None, "192"], ids=["whole_device", "quarter_of_the_groups"])
@pytest.mark.parametrize("shape,rule", SHAPE_RULES, ids=[f"N{s[0]}_R{s[1]}-{r}" for s, r in SHAPE_RULES])
def test_results_do_not_depend_on_the_start(shape, rule, reserve, monkeypatch):
    N, R, gw = shape
    # (the case is laid out against the groups of THIS run; the set-up solves of a shared case ran on whatever grid)
    G = ngroups_of(gw, reserve)
    B = RULES[rule](G)
    cs = case(N, R, B)
    if reserve:
        monkeypatch.setenv("LO_OC_RESERVE_CUS", reserve)
    rounds = -(-B // G)
    try:
        runs = [solve_start(cs, OFF, order=1), solve_start(cs, ON, order=1), solve_start(cs, ON, order=2),
                solve_start(cs, GIVEN, CAP, order=1), solve_start(cs, GIVEN, CAP, order=2), solve_start(cs, AUTO)]
    finally:
        K.resident_start_debug(AUTO)
        K.resident_order_debug(0)
    torch.cuda.synchronize()
    per_xcd = G // 8
    most_steps = per_xcd - 1 - per_xcd // 2 if per_xcd > 1 else 0  # (the XCD's last group waits longest)
    auto = DELTA if rounds >= MIN_ROUNDS and most_steps <= MAX_STEPS else 0
    for (res, st), delta in zip(runs, [0, DELTA, DELTA, CAP, CAP, auto]):
        assert st["ngroups"] == G, (st, G)
        assert st["delta"] == delta, (st, delta, rounds)
    first = runs[0][0]
    for i, (res, st) in enumerate(runs[1:], 1):
        assert torch.equal(res.x, first.x), f"solve {i} ({st}): x depends on the start"
        assert res.mean_residual == first.mean_residual, (i, st, res.mean_residual, first.mean_residual)
        assert res.iterations == first.iterations and res.tolerance_reached == first.tolerance_reached
        assert not res.nan_detected
    assert torch.equal(first.x, cs.refs[0].x) and first.mean_residual == cs.refs[0].mean_residual
    ex = et.woodbury(cs.C, cs.d, cs.rhs_host[0])
    err = float(((runs[3][0].x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
    print(f"{shape} {rule} B={B} G={G} reserve={reserve}: capped start against fp64 Woodbury {err:.3e}")
    assert err < 1e-4, err  # (the bound of tests/test_gpu_rs3_member_order.py)


@gpu
def test_injected_timeout_under_a_forced_start():
    """A launch that starts with its error word set, with every group waiting the cap: redone on the streaming engine;
    after the cool-down the solve runs resident again, with the start still forced, and returns the reference bits."""
    N, R, gw = SHAPES[1]
    cs = case(N, R, RULES["four_rounds"](ngroups_of(gw, "192")))
    ex = et.woodbury(cs.C, cs.d, cs.rhs_host[0])
    try:
        ref, st = solve_start(cs, GIVEN, CAP)
        assert st["delta"] == CAP and torch.equal(ref.x, cs.refs[0].x)
        s0 = K.resident_status()
        K.inject_resident_timeouts(1)
        hit = cs.solve(cs.rhs[0])
        e = K.cg_last_executed()
        s1 = K.resident_status()
        assert not e["resident"] and e["streaming_iterations"] >= 11, e
        assert s1["timeouts"] == s0["timeouts"] + 1 and s1["cooldown"] > 0
        assert K.resident_start_debug()["delta"] == CAP  # (the injected launch itself ran with the start)
        assert hit.iterations == ref.iterations
        err = float(((hit.x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
        assert err < 1e-4, err  # (another engine: the same solution, not the same bits)
        for _ in range(s1["cooldown"] - 1):
            cs.solve(cs.rhs[0])
        res, cleared = cs.solve_owned(cs.rhs[0])
        assert cleared == 1, "the launch behind a timed-out one must clear the buffer"
        assert K.resident_start_debug()["delta"] == CAP
        assert torch.equal(res.x, ref.x) and res.mean_residual == ref.mean_residual
    finally:
        K.resident_start_debug(AUTO)
        K.inject_resident_timeouts(0)


# ---- without a GPU ----
def test_the_delay_rule_against_a_table():
    d = K.resident_start_delay
    # the headline launch: 512 members in 64 groups, 8 per XCD, 8 rounds -- linear inside each dispatch wave (local
    # indices 0 .. 3 and 4 .. 7), XCD by XCD
    assert [d(AUTO, 0, 512, 64, g) for g in range(64)] == [0, 200, 400, 600, 0, 200, 400, 600] * 8
    # the rounds rule at 64 groups: nothing up to five rounds, the committed delay from six on
    for B, delta in ((0, 0), (1, 0), (64, 0), (128, 0), (129, 0), (256, 0), (320, 0), (321, 200), (384, 200), (4096, 200)):
        assert [d(AUTO, 0, B, 64, g) for g in (0, 1, 3, 4, 7, 63)] == [0, delta, 3 * delta, 0, 3 * delta, 3 * delta], B
    # the layout rule at eight rounds: automatic only where no group waits more than three steps
    #   groups per XCD:      1      2       4       7       8       9       16       32       64
    for ngroups, last in ((8, 0), (16, 0), (32, 200), (56, 600), (64, 600), (72, 0), (128, 0), (256, 0), (512, 0)):
        assert d(AUTO, 0, 8 * ngroups, ngroups, ngroups - 1) == last, ngroups
        assert d(AUTO, 0, 8 * ngroups, ngroups, 0) == 0
    assert [d(AUTO, 0, 448, 56, g) for g in range(7)] == [0, 200, 400, 0, 200, 400, 600]  # (7 per XCD: waves of 3 and 4)
    # forced: off, the committed delay whatever the rounds and the layout, a given delta
    assert [d(OFF, 0, 512, 64, g) for g in (0, 3, 63)] == [0, 0, 0]
    assert [d(ON, 0, 64, 64, g) for g in (0, 3, 5, 63)] == [0, 600, 200, 600]
    assert [d(GIVEN, 25, 64, 64, g) for g in range(10)] == [0, 25, 50, 75, 0, 25, 50, 75, 0, 25]
    assert d(GIVEN, 0, 512, 64, 7) == 0
    # one group per XCD (groups of 32 workgroups on 256 CUs): local index 0 everywhere, no wait
    for mode in (ON, GIVEN):
        assert [d(mode, 100, 64, 8, g) for g in range(8)] == [0] * 8
    # two groups per XCD: one group per dispatch wave, no wait either
    assert [d(GIVEN, 100, 64, 16, g) for g in range(4)] == [0, 0, 0, 0]
    # 64 groups per XCD (one workgroup per member), FORCED on: the waves are 32 groups long and run into the cap
    assert [d(ON, 0, 4096, 512, g) for g in (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 511)] == [0, 200, 600, 800, 800, 800, 0, 200, 800, 0, 800]
    # out of range
    assert d(4, 0, 512, 64, 0) == -1 and d(AUTO, 0, 512, 64, 64) == -1 and d(AUTO, 0, 512, 60, 0) == -1


def test_the_cap():
    d = K.resident_start_delay
    assert K.RESIDENT_START_CAP_TICKS == CAP
    for delta in (CAP, CAP + 1, 5000, 65535, 65536 + 7, 2 ** 31 - 1):
        waits = [d(GIVEN, delta, 512, 64, g) for g in range(64)]
        assert max(waits) == CAP and min(waits) == 0, (delta, waits)
    assert all(d(GIVEN, -5, 512, 64, g) == 0 for g in range(64))
    assert max(d(ON, 0, 10 ** 9, 512, g) for g in range(512)) == CAP


def test_binding_of_the_start_exports():
    assert _hip.ABI_VERSION >= 35
    for name, n in (("lo_resident_start_debug", 3), ("lo_resident_start_delay", 5)):
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS
        restype, argtypes = _hip._PROTOTYPES[name]
        assert restype is ctypes.c_int and len(argtypes) == n
        assert hasattr(ctypes.CDLL(_hip.lib_path()), name), "liblo_amd.so does not export " + name
    assert _hip._PROTOTYPES["lo_resident_start_debug"][1][2] is ctypes.POINTER(ctypes.c_uint32)
    assert _hip.load().lo_abi_version() == _hip.ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lo_amd.h")).read()
    assert "int lo_resident_start_debug(int32_t mode, int32_t delta_ticks, uint32_t* out);" in hdr
    assert "int lo_resident_start_delay(int32_t mode, int32_t delta_ticks, int64_t B, int32_t ngroups, int32_t grp);" in hdr
