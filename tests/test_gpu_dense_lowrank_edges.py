"""lo_matvec_f32 on dense and low-rank operators at every dispatch border, on the MI355X, against int64 references at
tolerance zero.

The inputs (tests/dense_lowrank_edge_cases.py) are integers from {+-1, +-2, +-3} with diagonals from {1, 2, 3}: every sum
the kernels form is an integer below 2^24, exact in float32 in any order, so each result must equal the reference bit for
bit (`E.exact`); tests/test_dense_lowrank_edges_cpu.py shows that the tables reach the branches below and that the sums
stay in range.  The C entry point is driven directly on the test's own buffers: K, C, v and d sit between NaN bands (a
read beyond an operand poisons the result; the base that is 4 mod 16 starts one float into its band), y sits between
sentinel floats, the workspace has exactly the reported size, is filled with 0xFF bytes (NaN) before every call -- a
partial nobody wrote poisons the result -- and sits between guard bytes.  Every call is made twice (same bits), and the
profiler's report of each call is exactly the kernels, with their launch counts, `E.route(case)` predicts: no other
code can have served a case.

Which test reaches what:
  dense valu     k_dense_mv<1 | 2 | 4>, both N & 3 branches, N = 1 .. 255 (N < 4: rows clamped to N - 1), two and three
                 4-column passes, c = 1 at N = 256, 257, 1027, 32 rows per workgroup, the float4 loads of c = 1 on a base
                 that is 4 mod 16
  dense mfma16   k_dense_mv_mfma16<NV = 0 .. 4, UNAL = false | true>: UNAL by a ragged last tile, by rows that are not
                 16-byte aligned (N = 257, 258, 319, 321) and by the base pointer alone (N = 256, 320)
  dense splitk   2 equal slices; 640 + 460 and 640 + 387 (unaligned rows); 3 equal; 5 with a last one of 1 column; 7 sized
                 and 6 launched; 3 members; the batch that switches the split off and the one before; the pad_lds launch
  dense mfma32   k_dense_mv_mfma at c = 21 .. 32 and with two and three column tiles (the last of 1 and of 20 columns),
                 full_rows on and off, the float4 loads on a base that is 4 mod 16
  lowrank valu   k_skinny_tn / k_skinny_nn<CT, RQ> for CT = 1, 2, 4, 8 and RQ = 1 .. 64, chunks behind the first, padded
                 copies at every width, S = 1, ragged last slices (329, 229 and 5 rows), N = 1 and 3; where the resident
                 kernel takes the shape, it too, with the same bits
  lowrank mfma   k_skinny_tn_mfma<NT = 1, 2, 4>, k_skinny_nn_mfma<KQ = 1 .. 16>, c = 9 .. 32, staged and direct tiles
  terms          the same operators as terms of a sum and under a mask; ranks whose padded width is refused"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import dense_lowrank_edge_cases as E

from linear_operator_amd import _hip as H
from linear_operator_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024          # sentinel floats before and after y
WS_GUARD = 4096       # guard bytes before and after the workspace
SENTINEL = -7777.25   # no integer: a result can never equal it
SWITCHES = ("LO_NO_RESIDENT_MV", "LO_MV_TEST_FALLBACK", "LO_DENSE_MFMA32", "LO_DENSE_OCC3")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # (a copy: the cases' arrays are read-only)


def banded(a, misaligned=False):
    """`a` on the device as a view into a flat buffer with GUARD NaN floats on either side: a read beyond the operand
    poisons the result.  `misaligned`: the view starts one float further in, so that its base is 4 mod 16."""
    a = np.asarray(a, np.float32)
    flat = torch.full((a.size + 2 * GUARD + 4,), float("nan"), dtype=torch.float32, device=DEV)
    off = GUARD + (1 if misaligned else 0)
    view = flat[off:off + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    return view


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(autouse=True)
def env():
    """Set / restore the switches the library reads at every launch; none is set when a test starts."""
    saved = {name: os.environ.pop(name, None) for name in SWITCHES}

    def set_(name, value):
        assert name in SWITCHES
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value

    yield set_
    for name, value in saved.items():
        os.environ.pop(name, None)
        if value is not None:
            os.environ[name] = value


class Buffers:
    """y [shape] between sentinel floats and a workspace of exactly ws_bytes between guard bytes."""

    def __init__(self, shape, ws_bytes):
        self.n, self.ws_bytes = int(np.prod(shape)), ws_bytes
        self.ybuf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.y = self.ybuf[GUARD:GUARD + self.n].view(*shape)
        self.wsbuf = torch.full((ws_bytes + 2 * WS_GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        self.ws = self.wsbuf[WS_GUARD:WS_GUARD + ws_bytes]

    def poison(self):
        self.y.fill_(SENTINEL)
        self.ws.fill_(0xFF)
        torch.cuda.synchronize()

    def untouched(self):
        return bool((self.ybuf == SENTINEL).all())

    def intact(self):
        g = self.ybuf
        return (bool((g[:GUARD] == SENTINEL).all()) and bool((g[GUARD + self.n:] == SENTINEL).all())
                and bool((self.wsbuf[:WS_GUARD] == 0x5A).all()) and bool((self.wsbuf[WS_GUARD + self.ws_bytes:] == 0x5A).all()))


@contextlib.contextmanager
def profiled(expected):
    """Assert which kernels ran inside the block, and how many launches of each: {profiler name: launches}."""
    torch.cuda.synchronize()
    H.prof_enable(True)
    H.prof_report()
    try:
        yield
        torch.cuda.synchronize()
        ran = {name: launches for name, (launches, _) in H.prof_report().items()}
    finally:
        H.prof_enable(False)
    assert ran == dict(expected), (dict(expected), ran)


def call(desc, v, buf):
    s = desc.c_struct()
    c = v.shape[-1]
    return H.load().lo_matvec_f32(ctypes.byref(s), H.ptr(v), H.ptr(buf.y), c, H.ptr(buf.ws), buf.ws_bytes, H.stream_ptr(v.device))


def product(desc, v, kernels, ref, *what, least_bytes=0):
    """Two calls of lo_matvec_f32 on poisoned buffers of exactly the reported size: the kernels of `kernels` and no
    others, the reference bit for bit both times, the guards intact."""
    s = desc.c_struct()
    need = int(H.load().lo_matvec_workspace_bytes(ctypes.byref(s), v.shape[-1]))
    assert need >= E.PLAN_TAIL + least_bytes, (need, least_bytes)
    buf = Buffers(tuple(v.shape), need)
    outs = []
    for _ in range(2):
        buf.poison()
        with profiled(kernels):
            assert call(desc, v, buf) == 0, what
        assert buf.intact(), ("a write outside y or outside the workspace", *what)
        outs.append(buf.y.clone())
    assert E.exact(host(outs[0]), ref), f"{what}: {E.mismatches(host(outs[0]), ref)}"
    assert torch.equal(bits(outs[0]), bits(outs[1])), ("two calls differ", *what)
    return outs[0]


def diag_args(data, mode):
    d = E.diag_of(data, mode)
    return (None if d is None else banded(d)), mode == "const"


# ---- dense -------------------------------------------------------------------------------------------------------------------
def run_dense(k):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = E.route(k, cus=cus)
    if E.route(k).get("pad_lds") and not r["pad_lds"]:
        pytest.skip(f"the pad_lds launch needs 3 cus < {np.prod(r['grid'])} <= 4 cus workgroups; this device has {cus} compute units")
    data = E.dense_data(k.B, k.N, k.c)
    d, const = diag_args(data, k.diag)
    desc = K.dense_diag_descriptor(banded(data["K"], k.misaligned), d, const_diag=const)
    assert desc.kind == H.LO_OP_DENSE_DIAG and (desc.B, desc.N) == (k.B, k.N)
    assert desc.A0.data_ptr() % 16 == (4 if k.misaligned else 0), "the operand's alignment did not survive the descriptor"
    product(desc, banded(data["v"]), r["kernels"], E.reference(k), "dense", k.id, least_bytes=r["workspace"])


def cases(table, group):
    return pytest.mark.parametrize("k", [k for k in table if k.group == group], ids=lambda k: k.id)


@cases(E.DENSE, "valu")
def test_dense_valu(k):
    run_dense(k)


@cases(E.DENSE, "mfma16")
def test_dense_mfma16(k):
    run_dense(k)


@cases(E.DENSE, "splitk")
def test_dense_splitk(k):
    run_dense(k)


@cases(E.DENSE, "mfma32")
def test_dense_mfma32(k):
    run_dense(k)


# ---- low-rank ----------------------------------------------------------------------------------------------------------------
def run_lowrank(k, env):
    data = E.lowrank_data(k.B, k.N, k.R, k.c)
    d, const = diag_args(data, k.diag)
    desc = K.lowrank_diag_descriptor(banded(data["C"]), d, const_diag=const)
    assert desc.kind == H.LO_OP_LOWRANK_DIAG and (desc.B, desc.N, desc.R) == (k.B, k.N, k.R)
    v, ref, r = banded(data["v"]), E.reference(k), E.route(k)
    env("LO_NO_RESIDENT_MV", "1")
    two_pass = product(desc, v, r["kernels"], ref, "low-rank, two passes", k.id, least_bytes=r["workspace"])
    env("LO_NO_RESIDENT_MV", None)
    if E.lowrank_mv_eligible(r["R4"], k.N, k.c):
        K.set_onchip_cg(True)   # (the default; it also ends a cool-down an earlier test may have left)
        resident = product(desc, v, E.route(k, resident=True)["kernels"], ref, "low-rank, resident", k.id)
        assert torch.equal(bits(resident), bits(two_pass))
    else:   # a shape the resident kernel does not take: the same two passes without the switch
        product(desc, v, r["kernels"], ref, "low-rank, two passes by shape", k.id)


@cases(E.LOWRANK, "valu")
def test_lowrank_valu(k, env):
    run_lowrank(k, env)


@cases(E.LOWRANK, "mfma")
def test_lowrank_mfma(k, env):
    run_lowrank(k, env)


@pytest.mark.parametrize("R", E.REFUSED_R)
def test_a_rank_beyond_the_widest_kernel_is_refused(R):
    """padded_rank(R) > 256: LO_ERR_UNSUPPORTED, y untouched, nothing launched."""
    B, N, c = 2, 300, 3
    C, v = dev(E.ints(E.rng(7, R), (B, N, R))), dev(E.ints(E.rng(8, R), (B, N, c)))
    desc = K.lowrank_diag_descriptor(C, dev(E.full_diag(E.rng(9, R), B, N)))
    buf = Buffers((B, N, c), 1 << 20)
    buf.poison()
    with profiled({}):
        assert call(desc, v, buf) == H.LO_ERR_UNSUPPORTED
    assert buf.untouched() and buf.intact() and bool((buf.ws == 0xFF).all())


# ---- as terms of a sum and under a mask ------------------------------------------------------------------------------------
def term_data():
    B, N, R = E.TERM_B, E.TERM_N, E.TERM_R
    return E.dense_data(B, N, max(E.TERM_COLS)), E.lowrank_data(B, N, R, max(E.TERM_COLS))


@pytest.mark.parametrize("c", E.TERM_COLS)
def test_dense_and_lowrank_as_terms_of_a_sum(c, env):
    """C C^T + K + d at N = 321: the low-rank term's padded copy and partials, the dense term on a ragged last tile, one
    diagonal on the first term's epilogue (the low-rank term comes first).  The reference is the sum of the two int64
    products; the kernels are each term's own route and one vec_axpy1 (E.sum_kernels)."""
    dn, lr = term_data()
    v_h = dn["v"][..., :c]
    ref = E.dense_product(dn["K"], v_h) + E.lowrank_product(lr["C"], v_h) + E.diag_term(dn["d_full"], v_h, "full")
    terms = (K.lowrank_diag_descriptor(banded(lr["C"]), None), K.dense_diag_descriptor(banded(dn["K"]), None))
    desc = K.sum_descriptor(terms, banded(dn["d_full"]))
    assert desc.kind == H.LO_OP_SUM
    v = banded(v_h)
    env("LO_NO_RESIDENT_MV", "1")
    a = product(desc, v, E.sum_kernels(c, resident=False), ref, "sum, two passes", c)
    env("LO_NO_RESIDENT_MV", None)
    K.set_onchip_cg(True)
    b = product(desc, v, E.sum_kernels(c, resident=True), ref, "sum", c)
    assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("c", E.TERM_COLS)
@pytest.mark.parametrize("base", ("dense", "lowrank"))
def test_dense_and_lowrank_under_a_mask(base, c):
    """S A S^T v + d o v with 257 of 321 rows kept: the base's own product at N = 321 on the expanded vector.  The
    reference is the product with the submatrix (dense), with the kept rows of C (low-rank)."""
    dn, lr = term_data()
    idx = E.mask_rows(E.TERM_N, E.MASK_KEEP)
    v_h = dn["v"][:, :E.MASK_KEEP, :c]
    d_h = dn["d_full"][:, :E.MASK_KEEP]
    if base == "dense":
        ref = E.dense_product(dn["K"][:, idx][:, :, idx], v_h)
        base_desc = K.dense_diag_descriptor(banded(dn["K"]), None)
    else:
        ref = E.lowrank_product(lr["C"][:, idx], v_h)
        base_desc = K.lowrank_diag_descriptor(banded(lr["C"]), None)
    ref = ref + E.diag_term(d_h, v_h, "full")
    desc = K.masked_descriptor(base_desc, dev(idx), banded(d_h))
    assert desc is not None and desc.kind == H.LO_OP_MASKED and desc.N == E.MASK_KEEP
    product(desc, banded(v_h), E.masked_kernels(base, c), ref, "masked", base, c)
