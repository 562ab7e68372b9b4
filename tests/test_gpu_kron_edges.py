"""lo_matvec_f32 / lo_matvec_f64 on Kronecker operators at every engine and tile edge, on the MI355X, against float64
references at tolerance zero.

The inputs (tests/kron_edge_cases.py) are integers from {+-1, +-2, +-3} with diagonals from {1, 2, 3} and factors that
are NOT symmetric: every sum the kernels form is an integer below 2^24, exact in float32 in any order, so each result
must equal the reference bit for bit (`E.exact`) and must differ from the product with either factor transposed;
tests/test_kron_edges_cpu.py shows that the tables reach the edges below and that the sums stay in range.  The C entry
points are driven directly on the test's own buffers: K1, K2, v and d sit between NaN bands (a read beyond an operand
poisons the result), y sits between sentinel values, the workspace has exactly the reported size, is filled with 0xFF
bytes (NaN) before every call and sits between guard bytes.  Every call is made twice (same bits), and the profiler's
report of each call is exactly the kernels, with their launch counts, `E.route(case)` predicts.

Which test reaches what:
  valu     k_gemm twice (+ vec_add_diag): one to three row tiles, up to 65 column tiles, ragged BK slabs in either pass,
           n2 c = 63 / 64 / 65, both staging orders of A (c = 1 / c > 1) and of B (n2 = 1), c = 65 on matrix-core factors,
           one factor the matrix cores refuse
  mfma     k_kron_nt_mfma<EPI, GUARD> twice: {128, 256, 384}^2, guarded sizes one step past / before a tile or slab,
           mixed aligned / ragged pairs, B = 1, 7, 8, 9 (the XCD mapping), the epilogue's three diagonal modes
  cols     k_kron_cols -> two GEMMs with a_div = c -> k_kron_cols: c = 2 .. 64 (66 560 bytes of dynamic LDS at 64),
           B c = 3, 8, 9, 51, a ragged last block of 16 rows, the diagonal on the way back
  fused    k_kron_fused<8,4 | 8,0 | 4,2 | 4,0> at the gate (95 / 96) and at B = 49, 97; each case again with
           LO_NO_KRON_FUSED (two launches at these batches), same bits
  f64      k64_kron_gemm: c = 7 / 8 (kfast), Q = 31 / 32 / 33, n = 1 .. 65; a sum of two terms (accumulate = 1)
  164 table cases: cols, fused and f64 cross every shape with the three diagonal modes; valu and mfma, whose cross would
  exceed 40 cases, give every shape at least one mode and every mode to every instantiation
  misaligned bases, one CG step on the fused dot partials of each matrix-core route, the refused B c > 65535"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import cases
import kron_edge_cases as E
from test_gpu_kernel_op import ERR_FLOOR, REF_FACTOR

from linear_operator_amd import _hip as H
from linear_operator_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024          # NaN / sentinel elements before and after an operand / y
WS_GUARD = 4096       # guard bytes before and after the workspace
SENTINEL = -7777.25   # no integer: a result can never equal it


def tdtype(f64):
    return torch.float64 if f64 else torch.float32


def banded(a, f64=False, misaligned=False):
    """`a` on the device as a view into a flat buffer with GUARD NaNs on either side: a read beyond the operand poisons
    the result.  `misaligned` (float32): the view starts one float further in, so that its base is 4 mod 16."""
    a = np.asarray(a, np.float64 if f64 else np.float32)
    flat = torch.full((a.size + 2 * GUARD + 4,), float("nan"), dtype=tdtype(f64), device=DEV)
    off = GUARD + (1 if misaligned else 0)
    view = flat[off:off + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(np.array(a, order="C")))
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return view


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    """The gate reads LO_NO_KRON_FUSED at every call; it is not set when a test starts."""
    monkeypatch.delenv("LO_NO_KRON_FUSED", raising=False)


class Buffers:
    """y [shape] between sentinel values and a workspace of exactly ws_bytes between guard bytes."""

    def __init__(self, shape, ws_bytes, f64=False, misaligned=False):
        self.n, self.ws_bytes = int(np.prod(shape)), ws_bytes
        self.off = GUARD + (1 if misaligned else 0)
        self.ybuf = torch.full((self.n + 2 * GUARD + 4,), SENTINEL, dtype=tdtype(f64), device=DEV)
        self.y = self.ybuf[self.off:self.off + self.n].view(*shape)
        assert self.y.data_ptr() % 16 == (4 if misaligned else 0)
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
        return (bool((g[:self.off] == SENTINEL).all()) and bool((g[self.off + self.n:] == SENTINEL).all())
                and bool((self.wsbuf[:WS_GUARD] == 0x5A).all()) and bool((self.wsbuf[WS_GUARD + self.ws_bytes:] == 0x5A).all()))


def report():
    return {name: launches for name, (launches, _) in H.prof_report().items()}


@contextlib.contextmanager
def profiled(expected):
    """Assert which kernels ran inside the block, and how many launches of each: {profiler name: launches}."""
    torch.cuda.synchronize()
    H.prof_enable(True)
    H.prof_report()
    try:
        yield
        torch.cuda.synchronize()
        ran = report()
    finally:
        H.prof_enable(False)
    assert ran == dict(expected), (dict(expected), ran)


def call(desc, v, buf, f64=False):
    s = desc.c_struct(tdtype(f64))
    fn = H.load().lo_matvec_f64 if f64 else H.load().lo_matvec_f32
    return fn(ctypes.byref(s), H.ptr(v), H.ptr(buf.y), v.shape[-1], H.ptr(buf.ws), buf.ws_bytes, H.stream_ptr(v.device))


def product(desc, v, kernels, ref, want_bytes, *what, f64=False, y_misaligned=False, wrong=()):
    """Two calls on poisoned buffers of exactly the reported size: the kernels of `kernels` and no others, the
    reference bit for bit both times, the guards intact, and none of the `wrong` references."""
    s = desc.c_struct(tdtype(f64))
    sizer = H.load().lo_matvec_f64_workspace_bytes if f64 else H.load().lo_matvec_workspace_bytes
    need = int(sizer(ctypes.byref(s), v.shape[-1]))
    assert need == want_bytes, (need, want_bytes)
    buf = Buffers(tuple(v.shape), need, f64, y_misaligned)
    outs = []
    for _ in range(2):
        buf.poison()
        with profiled(kernels):
            assert call(desc, v, buf, f64) == 0, what
        assert buf.intact(), ("a write outside y or outside the workspace", *what)
        outs.append(buf.y.clone())
    got = host(outs[0])
    assert E.exact(got, ref), f"{what}: {E.mismatches(got, ref)}"
    assert torch.equal(bits(outs[0]), bits(outs[1])), ("two calls differ", *what)
    for name, w in wrong:
        assert not np.array_equal(got, w), (f"the result is the product with {name} transposed", *what)
    return outs[0]


def descriptor(k, dat, misaligned=False):
    d = E.diag_of(dat, k.diag)
    desc = K.kron_diag_descriptor(banded(dat["K1"], k.f64, misaligned), banded(dat["K2"], k.f64, misaligned),
                                  None if d is None else banded(d, k.f64), const_diag=k.diag == "const", dtype=tdtype(k.f64))
    assert desc.kind == H.LO_OP_KRON_DIAG and (desc.B, desc.N, desc.R, desc.n2) == (k.B, k.N, k.n1, k.n2)
    # (a contiguous view is handed on as it is: the descriptor layer makes no aligned copy of it)
    assert desc.A0.data_ptr() % 16 == desc.A1.data_ptr() % 16 == (4 if misaligned else 0)
    return desc


def transposed_refs(k):
    """The references a factor read transposed would give, for the factors that have more than one row."""
    return [(name, E.reference(k, which)) for name, which, n in (("K1", "Kv_t1", k.n1), ("K2", "Kv_t2", k.n2)) if n > 1]


def run(k, no_fused=False, misaligned=False, y_misaligned=False):
    dat, r = E.case_data(k), E.route(k, no_fused=no_fused)
    desc = descriptor(k, dat, misaligned)
    v = banded(dat["v"], k.f64, misaligned)
    return product(desc, v, r["kernels"], E.reference(k), k.workspace_bytes, r["engine"], sorted(r["inst"]), k.id,
                   f64=k.f64, y_misaligned=y_misaligned, wrong=transposed_refs(k)), desc, v


def table(name):
    return pytest.mark.parametrize("k", E.TABLES[name], ids=lambda k: k.id)


# ---- exact products --------------------------------------------------------------------------------------------------------
@table("valu")
def test_valu(k):
    run(k)


@table("mfma")
def test_mfma_two_launches(k):
    run(k)


@table("cols")
def test_mfma_columns(k):
    run(k)


@table("fused")
def test_fused_and_its_two_launch_twin(k, monkeypatch):
    """Every case with and without LO_NO_KRON_FUSED: one launch (two at B = 95, below the gate), then the two launches
    at the same batch.  Both equal the reference, and therefore each other."""
    one, _, _ = run(k)
    monkeypatch.setenv("LO_NO_KRON_FUSED", "1")
    two, _, _ = run(k, no_fused=True)
    assert torch.equal(bits(one), bits(two))


@table("f64")
def test_float64(k):
    """k64_kron_gemm has no profiler scope, so `route` predicts no kernel name for a float64 case: the profiler
    assertion here only shows that no float32 kernel ran, it is no check of the route.  What pins the kernel is the
    exact product at the shapes of the table."""
    y, desc, v = run(k)
    assert torch.equal(bits(K.matvec(desc, v)), bits(y))   # the public path: the same entry point on its own workspace


@pytest.mark.parametrize("c", E.SUM_COLS)
def test_float64_sum_of_two_kronecker_terms(c):
    """K1 (x) K2 + K3 (x) K4 + d as a float64 LO_OP_SUM: the second term runs k64_kron_gemm with accumulate = 1 and
    carries the diagonal.  The entries are exact in float64."""
    B, (a, b) = E.SUM_B, E.SUM_TERMS
    da, db = E.data(B, a[0], a[1], c, seed=1), E.data(B, b[0], b[1], c, seed=2)
    v_h = da["v"]
    ref = da["Kv"] + E.product(db["K1"], db["K2"], v_h) + E.diag_term(da["d_full"], v_h, "full")
    terms = tuple(K.kron_diag_descriptor(banded(d["K1"], True), banded(d["K2"], True), None, dtype=torch.float64)
                  for d in (da, db))
    desc = K.sum_descriptor(terms, banded(da["d_full"], True), dtype=torch.float64)
    assert desc.kind == H.LO_OP_SUM
    N = a[0] * a[1]
    wrong = [("the second term's K1", da["Kv"] + E.product(db["K1"].transpose(0, 2, 1), db["K2"], v_h)
              + E.diag_term(da["d_full"], v_h, "full")), ("no accumulation", ref - da["Kv"])]
    product(desc, banded(v_h, True), {}, ref, E.F64_TAIL + 8 * B * N * c, "float64 sum", c, f64=True, wrong=wrong)


# ---- misaligned bases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("y_too", (False, True), ids=("operands", "operands-and-y"))
@pytest.mark.parametrize("k", E.MISALIGNED, ids=lambda k: f"{k.group}-{k.id}")
def test_bases_four_bytes_off_a_16_byte_boundary(k, y_too):
    """K1, K2 and v start at element 1 of a flat buffer (the matrix-core engines load float4 from them), then y too.  The
    descriptor layer hands such views on without a copy (`descriptor` asserts the pointers)."""
    run(k, misaligned=True, y_misaligned=y_too)


# ---- the fused dot partials: one CG step ---------------------------------------------------------------------------------
def member_rel(x, want):
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    return float((np.linalg.norm((x - want).reshape(x.shape[0], -1), axis=1)
                  / np.linalg.norm(want.reshape(x.shape[0], -1), axis=1)).max())


@pytest.mark.parametrize("diag", ("const", "full"))
@pytest.mark.parametrize("n1,n2,B", E.CG_STEP, ids=lambda n: str(n))
def test_one_cg_step_reads_the_epilogues_dot_partials(n1, n2, B, diag):
    """x after one step from x0 = 0 without a preconditioner is alpha rhs with alpha = (r.r) / (r.A r): p.Ap comes from
    the partials the matrix-core epilogue (two launches: aligned and guarded) or the fused kernel writes per tile, in the
    layout of kron_S_dot; a dropped or doubled tile moves alpha by at least 1 / (tiles + 1) >= 1/7.  No engine that forms
    p.Ap itself takes these shapes: the streaming loop runs the matvec with its epilogue at all four, and the profiler
    shows the route's kernel inside the solve.  The bound: the worst member's relative error of x is at most REF_FACTOR
    times the larger of ERR_FLOOR and the worst member's error of the same formula in torch float32 on the dense
    torch.kron matrix, member by member."""
    K1, K2, sig, rhs = cases.kron_factors(9900 + n1 + n2 + B, B, n1, n2, 1, sigma=0.05)
    N = n1 * n2
    d = sig[:, 0] if diag == "const" else (0.05 + 0.1 * E.rng(7, n1, n2, B).random((B, N))).astype(np.float32)
    k = E.Kron("cg", n1, n2, 1, B, diag)
    Ar = E.product(K1, K2, rhs) + E.diag_term(d, rhs, diag)
    r64 = rhs.astype(np.float64)
    alpha = (r64 * r64).sum(axis=(1, 2)) / (r64 * Ar).sum(axis=(1, 2))
    want = alpha[:, None, None] * r64
    t1, t2, tr, td = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (K1, K2, rhs, d))
    ref = torch.empty_like(tr)
    for b in range(B):   # the same formula in float32 on the dense matrix, a member at a time
        A = torch.kron(t1[b], t2[b])
        Arb = A @ tr[b] + (td[b][:, None] if diag == "full" else td[b]) * tr[b]
        del A
        ref[b] = ((tr[b] * tr[b]).sum() / (tr[b] * Arb).sum()) * tr[b]
    ref_err = max(member_rel(host(ref), want), ERR_FLOOR)
    desc = K.kron_diag_descriptor(t1, t2, td, const_diag=diag == "const")
    torch.cuda.synchronize()
    H.prof_enable(True)
    H.prof_report()
    try:
        res = K.cg_solve(desc, tr, tolerance=1e-6, max_iter=1)
        torch.cuda.synchronize()
        ran = report()
    finally:
        H.prof_enable(False)
    assert res.iterations == 1 and not res.nan_detected
    for name, launches in E.route(k)["kernels"].items():
        assert ran.get(name) == launches, (name, ran)
    assert ran.get("vec_dot_part", 0) <= 2, ran   # (the norms of cg_init only: p.Ap is the epilogue's)
    err = member_rel(host(res.x), want)
    print(f"cg step {n1}x{n2} B={B} {diag} ({E.route(k)['engine']}): err {err:.3e} torch fp32 {ref_err:.3e} "
          f"ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (err, ref_err)


# ---- refusal -----------------------------------------------------------------------------------------------------------------
def test_a_batch_of_columns_beyond_the_grid_is_refused():
    """B c = 65552 > 65535 on the VALU route (1 (x) 1, B = 3856, c = 17): LO_ERR_UNSUPPORTED, y keeps its sentinels, the
    workspace guards are intact.  (The first pass has no such batch and may have run into the workspace.)"""
    k = E.REFUSED
    assert E.route(k)["refused"]
    dat = E.case_data(k)
    desc = descriptor(k, dat)
    buf = Buffers((k.B, k.N, k.c), k.workspace_bytes)
    buf.poison()
    torch.cuda.synchronize()
    H.prof_enable(True)
    H.prof_report()
    try:
        rc = call(desc, banded(dat["v"]), buf)
        torch.cuda.synchronize()
        ran = report()
    finally:
        H.prof_enable(False)
    assert rc == H.LO_ERR_UNSUPPORTED
    assert set(ran) <= {"kron_gemm"} and ran.get("kron_gemm", 0) <= 1, ran
    assert buf.untouched() and buf.intact()
