"""The headline solve sends its ticket in front of the last x pass (csrc/lo_rspace3.hip, csrc/lo_cg_close.h):
workgroup 0 of a group runs the closing step for the group's final member behind the iteration chain, the x pass follows.
When the solve returns, `info` is final and x is complete in stream order (include/lo_amd.h).

For every shape at which the new order can go wrong -- fewer members than groups (most groups count in behind the loop),
one group a round behind the others, four workgroups per member, one workgroup per member with a ragged last round, the
headline member shape:

  * consecutive solves repeat bit for bit, never clear the library's buffer, and meet the fp64 Woodbury solution;
  * a consumer enqueued straight behind the return sees all of x, on the solve's stream and on a stream that waits for it;
  * with peer buffers installed (the close stays behind the x pass) both buffers hold x, and the next solve is unchanged;
  * (fewest members only) an injected hand-off timeout is redone on the streaming engine and the next launch clears.

Without a GPU: the closing step's fused reduction adds the residual norms in the order of the four-call form it replaced.
"""
import numpy as np
import pytest
import torch

import cases

from linear_operator_amd import kernels as K  # noqa: E402

gpu = pytest.mark.gpu

SHAPES = [(3, 8192, 32), (9, 8192, 32), (64, 4096, 16), (65, 1000, 8), (64, 8192, 32)]
N_RHS = 5      # right-hand sides with their own reference each
N_REPEAT = 50


@pytest.fixture(autouse=True)
def _form_on_second_use():
    old = K.EIGFORM_AFTER_USES
    K.EIGFORM_AFTER_USES = 1
    if torch.cuda.is_available():
        K.set_onchip_cg(True)  # (ends any cool-down another test may have left)
    yield
    K.EIGFORM_AFTER_USES = old
    if torch.cuda.is_available():
        K.inject_resident_timeouts(0)
        K.peer_gather_set(())
        K.set_onchip_cg(True)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def woodbury(C, d, rhs):
    C64, d64, r64 = (torch.from_numpy(a).double().cuda() for a in (C, d, rhs))
    Cd = C64 / d64.unsqueeze(-1)
    cap = torch.eye(C64.shape[-1], dtype=torch.float64, device="cuda") + C64.mT @ Cd
    return r64 / d64.unsqueeze(-1) - Cd @ torch.linalg.solve(cap, C64.mT @ (r64 / d64.unsqueeze(-1)))


class Case:
    """One operator with its root-form preconditioner, already on the diagonal form (tests/test_gpu_epoch_handoff.py),
    N_RHS right-hand sides and, for each, the solve right after a forced clear of the library's buffer."""

    def __init__(self, seed, B, N, R):
        self.shape = (B, N, R)
        C, d, rhs = cases.lowrank_diag(seed, B, N, R, 1)
        self.C, self.d = C, d
        self.desc = K.lowrank_diag_descriptor(dev(C), dev(d))
        L, perm = K.pivoted_cholesky(self.desc, 15)
        self.pre = K.precond_build(L, dev(d), constant_diag=False, root=self.desc.A0, perm=perm)
        g = np.random.default_rng(seed + 1)
        self.rhs_host = [rhs] + [g.standard_normal(rhs.shape).astype(np.float32) for _ in range(N_RHS - 1)]
        self.rhs = [dev(r) for r in self.rhs_host]
        self.solve(self.rhs[0])  # first use: dense R-space form
        self.solve(self.rhs[0])  # second use: the cache gets the diagonal form
        assert torch.is_tensor(self.pre.RSD)
        self.refs = []
        for r in self.rhs:
            K.resident_handoff_debug(force_clear=True)
            res, cleared = self.solve_owned(r)
            assert cleared == 1
            torch.cuda.synchronize()
            self.refs.append(res)

    def solve(self, rhs):
        return K.cg_solve(self.desc, rhs, precond=self.pre, tolerance=1e-4)

    def solve_owned(self, rhs):
        """A solve that must run k_cg_rspace3 on the library's buffer: (result, buffer was cleared in front of it)."""
        s0 = K.resident_handoff_debug()
        res = self.solve(rhs)
        e = K.cg_last_executed()
        s1 = K.resident_handoff_debug()
        assert e["resident"] and e["rspace"] == "resident" and e["rspace_diag"] and e["lean"], e
        assert e["streaming_iterations"] == 0, e
        assert s1["launches"] == s0["launches"] + 1, "the solve did not run on the library's hand-off buffer"
        return res, s1["clears"] - s0["clears"]


_cases = {}


def case(shape):
    if shape not in _cases:
        _cases[shape] = Case(9100 + SHAPES.index(shape), *shape)
    return _cases[shape]


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_solves_repeat_never_clear_and_meet_the_closed_form(shape):
    cs = case(shape)
    first = cs.refs[0]
    ex = woodbury(cs.C, cs.d, cs.rhs_host[0])
    err = float(((first.x.double() - ex).norm(dim=-2) / ex.norm(dim=-2)).max())
    assert err < 1e-4, err  # (the bound of tests/test_gpu_eigform.py for this engine)
    for i in range(N_REPEAT):
        res, cleared = cs.solve_owned(cs.rhs[0])
        assert cleared == 0, f"solve {i} cleared the buffer"
        assert torch.equal(res.x, first.x), f"solve {i} differs"
        assert res.iterations == first.iterations and res.mean_residual == first.mean_residual


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_consumer_behind_the_return_sees_all_of_x(shape):
    cs = case(shape)
    for i in range(N_REPEAT):
        w = i % N_RHS
        rhs = cs.rhs[w].clone()  # (fresh tensors: the caching allocator hands a just-freed x to the next solve)
        res, cleared = cs.solve_owned(rhs)
        y = res.x.clone()  # no synchronisation in between
        torch.cuda.synchronize()
        assert cleared == 0
        assert torch.equal(y, res.x), f"solve {i}: the copy is not the solution"
        assert torch.equal(y, cs.refs[w].x), f"solve {i} differs from its reference"
        assert res.iterations == cs.refs[w].iterations and res.mean_residual == cs.refs[w].mean_residual
        del res, y, rhs


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_consumer_on_a_stream_that_waits_for_the_solves_sees_all_of_x(shape):
    cs = case(shape)
    s = torch.cuda.Stream()
    cur = torch.cuda.current_stream()
    for i in range(N_REPEAT):
        w = i % N_RHS
        rhs = cs.rhs[w].clone()
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            res, cleared = cs.solve_owned(rhs)
        rhs.record_stream(s)
        cur.wait_stream(s)
        res.x.record_stream(cur)
        y = res.x.clone()
        torch.cuda.synchronize()
        assert cleared == 0
        assert torch.equal(y, res.x), f"solve {i}: the copy is not the solution"
        assert torch.equal(y, cs.refs[w].x), f"solve {i} differs from its reference"
        del res, y, rhs


@gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_peer_buffers_hold_x_and_the_next_solve_is_unchanged(shape):
    cs = case(shape)
    B, N, _ = shape
    world, rank = 2, 1  # this rank's members sit at [rank * B, (rank + 1) * B) of a peer's buffer
    peers = [torch.zeros(world * B, N, device="cuda") for _ in range(2)]
    try:
        K.peer_gather_set(peers, rank * B)
        res, cleared = cs.solve_owned(cs.rhs[0])
        torch.cuda.synchronize()
        assert cleared == 0
        assert torch.equal(res.x, cs.refs[0].x)
        assert res.iterations == cs.refs[0].iterations and res.mean_residual == cs.refs[0].mean_residual
        for p in peers:
            assert torch.equal(p[rank * B:(rank + 1) * B], res.x[..., 0]), "a peer buffer does not hold x"
            assert float(p[:rank * B].abs().max()) == 0.0, "a peer's other slice was written"
    finally:
        K.peer_gather_set(())
    res, cleared = cs.solve_owned(cs.rhs[0])
    assert cleared == 0 and torch.equal(res.x, cs.refs[0].x)


@gpu
def test_injected_timeout_with_fewer_members_than_groups():
    cs = case(SHAPES[0])
    ref = cs.refs[0]
    s0 = K.resident_status()
    K.inject_resident_timeouts(1)
    hit = cs.solve(cs.rhs[0])  # the resident launch starts with its error word set: redone on the streaming engine
    e = K.cg_last_executed()
    s1 = K.resident_status()
    assert not e["resident"] and e["streaming_iterations"] >= 11, e
    assert s1["timeouts"] == s0["timeouts"] + 1 and s1["cooldown"] > 0
    assert hit.iterations == ref.iterations
    for _ in range(s1["cooldown"] - 1):  # the cool-down: fall-back engine
        cs.solve(cs.rhs[0])
        assert not K.cg_last_executed()["resident"]
    res, cleared = cs.solve_owned(cs.rhs[0])  # re-armed
    assert cleared == 1, "the launch behind a timed-out one must clear the buffer"
    assert torch.equal(res.x, ref.x)
    assert res.iterations == ref.iterations and res.mean_residual == ref.mean_residual
    s2 = K.resident_status()
    assert s2["timeouts"] == s0["timeouts"] + 1 and s2["cooldown"] == 0
    res, cleared = cs.solve_owned(cs.rhs[0])
    assert cleared == 0 and torch.equal(res.x, ref.x)


# ---- without a GPU: the addition order of the closing step's residual sum (csrc/lo_cg_close.h) ----
def _butterfly_32_to_1(v):
    """wave_sum: v += partner(lane ^ off) for off = 32, 16, .. 1, all 64 lanes of every wave at once (float32)."""
    v = v.copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ off]).astype(np.float32)
    return v


def _four_call_mean(r):
    """The form that was replaced: thread t adds members t, t + 256, .. one by one; block_sum256 (wave butterfly, lane 0
    of every wave to LDS, (w0 + w1) + (w2 + w3)); divided by B."""
    n, B = r.shape
    lsum = np.zeros((n, 256), np.float32)
    for i0 in range(0, B, 256):
        m = min(256, B - i0)
        lsum[:, :m] = (lsum[:, :m] + r[:, i0:i0 + m]).astype(np.float32)
    w = _butterfly_32_to_1(lsum.reshape(n, 4, 64))[:, :, 0]
    tot = ((w[:, 0] + w[:, 1]).astype(np.float32) + (w[:, 2] + w[:, 3]).astype(np.float32)).astype(np.float32)
    return (tot / np.float32(B)).astype(np.float32)


def _fused_mean(r, ck=4):
    """The fused form: a thread's granules arrive in rounds of ck (members i0 + 256 q, q ascending, tails masked), the
    wave butterfly leaves every lane with the wave's sum, wave 0 reads the four of them back."""
    n, B = r.shape
    lsum = np.zeros((n, 256), np.float32)
    t = np.arange(256)
    for i0 in range(0, B, ck * 256):
        for q in range(ck):
            idx = i0 + 256 * q + t
            ok = idx < B
            val = r[:, np.minimum(idx, B - 1)]  # (the clamped load of a masked tail is not added)
            lsum = np.where(ok, (lsum + val).astype(np.float32), lsum)
    w = _butterfly_32_to_1(lsum.reshape(n, 4, 64))
    assert (w == w[:, :, :1]).all()  # every lane of a wave carries the same bits
    red = w[:, :, 0]
    tot = ((red[:, 0] + red[:, 1]).astype(np.float32) + (red[:, 2] + red[:, 3]).astype(np.float32)).astype(np.float32)
    return (tot / np.float32(B)).astype(np.float32)


def test_fused_reduction_adds_in_the_order_of_the_four_calls():
    g = np.random.default_rng(9199)
    r = np.abs(g.standard_normal((1000, 512))).astype(np.float32) * np.float32(1e-6)
    r *= (10.0 ** g.uniform(-3, 3, size=(1000, 1))).astype(np.float32)  # (residual norms of very different sizes)
    a, b = _four_call_mean(r), _fused_mean(r)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # (and a batch that is no multiple of the round: B = 65, the ragged shape of the GPU tests)
    r65 = r[:, :65].copy()
    assert np.array_equal(_four_call_mean(r65).view(np.uint32), _fused_mean(r65).view(np.uint32))
