"""The kernels of csrc/lo_ski.hip at every tile edge, on the MI355X, against integer references at tolerance zero.

The inputs (tests/ski_edge_cases.py) are integers from {+-1, +-2, +-3} and weights from {1/4, 1/2, 3/4, 1}: every sum the
kernels form is exact in float32 in any order, so each result must equal the float64 reference bit for bit
(`E.exact`); tests/test_ski_edges_cpu.py shows that the tables reach the branches below, that the sums stay below 2^24
units, and that the checker tells a reference with one wrong term per branch from the right one.  The standalone entry
points are launched the way linear_operator_amd.kernels launches them (K._launch, the sizer's workspace) on operands
that sit between NaN guard bands: the bands and the inputs must keep their bits.  The profiler's classes of every call
are asserted, so no other code can have served a case.  One case is real-valued: the run-to-run bits of W^T v.

Which case reaches what:
  k_tz_mv       one slice, one k tile, `k < ke` on its only tile          tz (1, 1) (1, 2) (1, 255) (1, 256)
                two / three slices of one tile, the last of 1 or 5 rows   tz (1, 257) (1, 513) (1, 517)
                row guard `i < M` with RB = 2, 3, 5                        tz (1, 257) .. (171, 517)
                kchunk = 512: two k tiles per slice, last slice of 6       tz (40, 1030)
                kchunk = 768: three k tiles, last slice 262 = 256 + 6      tz (64, 1030)
                one slice of three k tiles, the last of 5                  tz (171, 517)
                far lags: every t[lag] is +-1 .. +-3 and t[k] != t[k - 1], so each entry of `win`, `dmin` and the
                `ad < M` guard changes the sum                             every tz shape
                CB = 1, 2, 4, 8, 16, 24, 32; cc < CB at cc = 3, 5, 9, 17, 25 (CB = 4, 8, 16, 24, 32); chunks at
                col0 = 32 (cc = 1, 8, 32) and col0 = 64                    c in E.TZ_COLS_ONE at B = 1; c = 1, 3, 33 batched
  k_tz_reduce   KS = 1, 2, 3; a second pass of the grid-stride loop        tz (64, 1030) and (171, 517) at c = 33
                LO_DIAG_FULL dd[e / c], LO_DIAG_CONST dd[e / (M c)], B > 1 the Toeplitz kind on every tz shape
  k_tz_bil      M < 256, M = 256, 257; S = 1, 2, 5; ichunk = 512, 768; a last i slice masked by `i < ie` under windows
                masked by `i < M`; lag 0 without a2                        bilinear on every tz shape
  k_interp      outside indices dropped; LO_DIAG_FULL / CONST with B = 3   interp outside-*; the SKI kind
                a second pass                                              wrap, c = 16
  k_csr_count / scan / fill / sort    segments of 0, 1, 64, 65, 200 entries; duplicates; outside indices (M + 5 would
                land in the next member's counts); second passes of count, fill and sort; M + 1 = 2 .. 16385 in the scan
                                                                           csr structure on clustered-*, duplicate-*, outside-*, wrap
  k_interp_t_wave   c = 1, 7; a second and fourth trip of `k += 64`        interp c = 1, 7 on clustered-N65, -N200, -M1
                a second pass                                              wrap, c = 1
                vdiv = 3                                                   bcast, c = 7
  k_interp_t_lane   c = 8, 9; a second pass                                interp c = 8, 9; wrap, c = 16
                vdiv = 3                                                   bcast, c = 8
  k_interp_vgrad    S = 1, 5; outside entries give 0; a second pass        vgrad on every interp case; wrap
  the SKI kind  scatter, product and gather chained, with and without a kept plan, W_r shared or separate, the three
                diagonal modes, indices outside the grid on both sides     ski (1, 257, 300, 4), (3, 517, 400, 4)"""
import contextlib

import numpy as np
import pytest
import torch

import ski_edge_cases as E

from linear_operator_amd import kernels as K

pytestmark = pytest.mark.gpu
GUARD = 1024   # sentinel floats before and after every guarded operand


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")   # (a copy: the cases' arrays are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def guarded(values, n):
    """A contiguous view of n floats in the middle of a 1-D buffer with GUARD sentinel floats (NaN) on either side,
    holding `values` (or the sentinel)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    if values is not None:
        buf[GUARD:GUARD + n] = values.reshape(-1)
    return buf, buf[GUARD:GUARD + n]


class Bands:
    """The operands of one launch: float inputs and outputs between NaN bands, index inputs beside a copy."""

    def __init__(self):
        self.kept, self.outs = [], []

    def fin(self, array):
        t = dev(np.asarray(array, np.float32))
        buf, view = guarded(t, t.numel())
        self.kept.append((buf, bits(buf).clone()))
        return view.view(t.shape)

    def iin(self, array):
        t = dev(array)
        self.kept.append((t, t.clone()))
        return t

    def out(self, *shape):
        n = int(np.prod(shape))
        buf, view = guarded(None, n)
        self.outs.append((buf, n))
        return view.view(*shape)

    def intact(self):
        torch.cuda.synchronize()
        sentinel = bits(torch.full((GUARD,), float("nan"), dtype=torch.float32, device="cuda"))
        for t, before in self.kept:
            if not torch.equal(bits(t) if t.dtype == torch.float32 else t, before):
                return False
        return all(torch.equal(bits(buf[:GUARD]), sentinel) and torch.equal(bits(buf[GUARD + n:]), sentinel)
                   for buf, n in self.outs)


@contextlib.contextmanager
def profiled(expected, exactly=True):
    """Assert which kernel classes ran inside the block."""
    K._hip.prof_enable(True)
    K._hip.prof_report()
    try:
        yield
        torch.cuda.synchronize()
        ran = set(K._hip.prof_report())
    finally:
        K._hip.prof_enable(False)
    assert set(expected) <= ran, (expected, ran)
    assert ran <= set(expected) if exactly else all(name.startswith("ski_") for name in ran), (expected, ran)


def check(got, ref, *what):
    assert E.exact(host(got), ref), f"{what}: {E.mismatches(host(got), ref)}"


# ---- the launches, as linear_operator_amd.kernels makes them, on guarded operands ----------------------------------------
def lib():
    return K._hip.load()


def toeplitz_mv(g, t, u):
    B, M, c = u.shape
    t, u, y = g.fin(t), g.fin(u), g.out(B, M, c)
    K._launch("lo_toeplitz_mv_f32", y.device, t, B, M, u, c, y, ws_bytes=lib().lo_toeplitz_workspace_bytes(B, M, c))
    return y


def toeplitz_bilinear(g, u, v):
    B, M, S = u.shape
    u, v, out = g.fin(u), g.fin(v), g.out(B, M)
    K._launch("lo_toeplitz_bilinear_f32", out.device, u, v, B, M, S, out,
              ws_bytes=lib().lo_toeplitz_workspace_bytes(B, M, 1))
    return out


def interp(g, idx, vals, u):
    (B, N, J), (M, c) = idx.shape, u.shape[1:]
    idx, vals, u, y = g.iin(idx), g.fin(vals), g.fin(u), g.out(B, N, c)
    K._launch("lo_interp_f32", y.device, idx, vals, B, N, J, M, u, c, y)
    return y


def interp_t(g, idx, vals, v, M):
    (B, N, J), c = idx.shape, v.shape[2]
    idx, vals, v, out = g.iin(idx), g.fin(vals), g.fin(v), g.out(B, M, c)
    K._launch("lo_interp_t_f32", out.device, idx, vals, B, N, J, M, v, c, out,
              ws_bytes=lib().lo_interp_t_workspace_bytes(B, N, J, M))
    return out


def interp_t_planned(g, plan, vals, v, M):
    (B, N, J), c = vals.shape, v.shape[2]
    vals, v, out = g.fin(vals), g.fin(v), g.out(B, M, c)
    K._launch("lo_interp_t_planned_f32", out.device, plan, vals, B, N, J, M, v, c, out)
    return out


def interp_t_bcast(g, plan, vals, v, M):
    (B, P, N, J), c = vals.shape, v.shape[2]
    vals, v, out = g.fin(vals), g.fin(v), g.out(B, P, M, c)
    K._launch("lo_interp_t_bcast_planned_f32", out.device, plan, vals, B, P, N, J, M, v, c, out)
    return out


def interp_values_grad(g, idx, lv, R):
    (B, N, J), (M, S) = idx.shape, R.shape[1:]
    idx, lv, R, out = g.iin(idx), g.fin(lv), g.fin(R), g.out(B, N, J)
    K._launch("lo_interp_values_grad_f32", out.device, idx, B, N, J, M, lv, R, S, out)
    return out


# ---- the Toeplitz product and the Toeplitz kind ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,M", E.TZ_SHAPES)
def test_toeplitz_product_is_exact(B, M):
    with profiled({"ski_toeplitz_mv"}):
        for c in E.tz_cols(B):
            t, u, d, ref = E.tz_case(B, M, c)
            g = Bands()
            check(toeplitz_mv(g, t, u), ref, "toeplitz_mv", B, M, c)
            assert g.intact(), ("toeplitz_mv wrote outside y or changed an input", B, M, c)
            g = Bands()
            td, ud = g.fin(t), g.fin(u)
            for mode, dd in (("none", None), ("full", d), ("const", E.const_diag(B))):
                desc = K.toeplitz_diag_descriptor(td, None if dd is None else g.fin(dd), const_diag=mode == "const")
                assert desc.kind == K._hip.LO_OP_TOEPLITZ_DIAG
                check(K.matvec(desc, ud), ref + E.diag_term(dd, u, mode), "toeplitz kind", B, M, c, mode)
            assert g.intact(), ("the Toeplitz kind changed an input", B, M, c)


@pytest.mark.parametrize("B,M", E.TZ_SHAPES)
def test_lag_correlation_is_exact(B, M):
    with profiled({"ski_toeplitz_bilinear"}):
        for S in E.BIL_S:
            u, v, ref = E.bil_case(B, M, S)
            g = Bands()
            check(toeplitz_bilinear(g, u, v), ref, "toeplitz_bilinear", B, M, S)
            assert g.intact(), ("toeplitz_bilinear wrote outside g or changed an input", B, M, S)


# ---- interpolation ---------------------------------------------------------------------------------------------------------
def interp_entry_points(name, columns, strides):
    """Every interpolation entry point on one case (its plan built once), exact and between intact bands."""
    idx, vals = E.interp_case(name)
    B, M, N, J = E.case_shape(name)
    plan = K.interp_plan_build(dev(idx), M)
    for c in columns:
        u, v = E.operand(name, "u", M, c), E.operand(name, "v", N, c)
        wtv = E.wt_ref(idx, vals, v, M)
        g = Bands()
        check(interp(g, idx, vals, u), E.w_ref(idx, vals, u), "interp", name, c)
        check(interp_t(g, idx, vals, v, M), wtv, "interp_t", name, c)
        check(interp_t_planned(g, plan, vals, v, M), wtv, "interp_t_planned", name, c)
        assert g.intact(), ("an interpolation kernel wrote outside its output or changed an input", name, c)
    for S in strides:
        lv, R = E.operand(name, "lv", N, S), E.operand(name, "R", M, S)
        g = Bands()
        check(interp_values_grad(g, idx, lv, R), E.vgrad_ref(idx, lv, R), "interp_values_grad", name, S)
        assert g.intact(), ("interp_values_grad wrote outside g or changed an input", name, S)
    return plan


def check_csr(plan, name):
    """The plan tensor read with the mirrored layout: counts, segment order, and the fill cursors at their ends."""
    idx, _ = E.interp_case(name)
    B, M, N, J = E.case_shape(name)
    assert plan.numel() == E.plan_bytes(B, N, J, M)
    got = E.plan_arrays(host(plan), B, N, J, M)
    ptr, ids = E.csr_ref(idx, M)
    assert np.array_equal(got["ptr"], ptr), name
    assert np.array_equal(got["cur"][:, :M], ptr[:, 1:]) and np.array_equal(got["cur"][:, M], ptr[:, M]), name
    for b in range(B):
        assert np.array_equal(got["ids"][b, :ptr[b, M]], ids[b]), (name, b)
        assert sorted(got["tmp"][b, :ptr[b, M]].tolist()) == sorted(ids[b].tolist()), (name, b)


INTERP_CLASSES = {"ski_interp", "ski_interp_t", "ski_csr_build", "ski_interp_vgrad"}


@pytest.mark.parametrize("name", [row[0] for row in E.INTERP_CASES])
def test_interpolation_is_exact(name):
    with profiled(INTERP_CLASSES):
        plan = interp_entry_points(name, E.INTERP_C, E.VGRAD_S)
    if name in E.CSR_CASES:
        check_csr(plan, name)


@pytest.mark.parametrize("name", [row[0] for row in E.INTERP_CASES])
def test_interp_t_bcast_is_exact(name):
    """P = 3 terms read one v: member b of the plan reads v[b / 3] (the `vdiv > 1` read), at c = 7 (a wave per output)
    and c = 8 (a lane per output)."""
    P = E.BCAST_P
    idx, vals = E.interp_case(name, 2 * P)
    _, M, N, J = E.case_shape(name)
    with profiled({"ski_csr_build", "ski_interp_t"}):
        plan = K.interp_plan_build(dev(idx), M)
        for c in E.BCAST_C:
            v = E.operand(name, "v", N, c, members=2)
            ref = E.wt_ref(idx, vals, v[np.arange(2 * P) // P], M).reshape(2, P, M, c)
            g = Bands()
            check(interp_t_bcast(g, plan, vals.reshape(2, P, N, J), v, M), ref, "interp_t_bcast", name, c)
            assert g.intact(), ("interp_t_bcast wrote outside its output or changed an input", name, c)


def test_the_wrap_case_is_exact():
    """B N J, B M, B M c and B N c beyond the caps of the grids: every grid-stride loop of the interpolation kernels
    makes a second pass."""
    with profiled(INTERP_CLASSES):
        plan = interp_entry_points("wrap", E.WRAP_C, (1,))
    check_csr(plan, "wrap")


# ---- the SKI kind end to end -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outside", (False, True), ids=("inside", "outside"))
@pytest.mark.parametrize("B,M,N,J", E.SKI_SHAPES)
def test_ski_kind_is_exact(B, M, N, J, outside):
    k = E.ski_case(B, M, N, J, outside)
    g = Bands()
    t, li, lv, ri, rv = g.fin(k["t"]), g.iin(k["li"]), g.fin(k["lv"]), g.iin(k["ri"]), g.fin(k["rv"])
    diags = {"none": (None, None), "full": (k["d_full"], g.fin(k["d_full"])), "const": (k["d_const"], g.fin(k["d_const"]))}
    plans = {}
    for c in E.SKI_C:
        v = E.operand(f"ski{B}-{M}-{outside}", "v", N, c, members=B)
        vd = g.fin(v)
        for shared in (True, False):
            r_i, r_v, rid, rvd = (k["li"], k["lv"], li, lv) if shared else (k["ri"], k["rv"], ri, rv)
            base = E.ski_ref(k["t"], k["li"], k["lv"], r_i, r_v, v, None, "none")
            for kept in (False, True):
                classes = {"ski_interp", "ski_interp_t", "ski_toeplitz_mv"} | (set() if kept else {"ski_csr_build"})
                if kept and shared not in plans:
                    plans[shared] = K.interp_plan_build(rid, M)
                with profiled(classes):
                    for mode, (dh, dd) in diags.items():
                        desc = K.ski_diag_descriptor(t, li, lv, rid, rvd, dd, const_diag=mode == "const",
                                                     right_plan=plans[shared] if kept else None)
                        assert desc.kind == K._hip.LO_OP_SKI_DIAG and (desc.interp[2] is desc.interp[0]) == shared
                        check(K.matvec(desc, vd), base + E.diag_term(dh, v, mode), "SKI kind", (B, M, N, J), c, mode,
                              "shared" if shared else "separate", "kept plan" if kept else "own plan")
        if outside:   # a row of nothing but outside entries on the left gives d o v alone
            desc = K.ski_diag_descriptor(t, li, lv, ri, rv, None)
            assert not host(K.matvec(desc, vd))[:, 0].any()
    assert g.intact(), "the SKI kind changed an input"


# ---- determinism where integers cannot show it -----------------------------------------------------------------------------
def col_err(y, ref):
    y = np.asarray(y, np.float64)
    return (np.linalg.norm(y - ref, axis=-2) / np.linalg.norm(ref, axis=-2)).max()


@pytest.mark.parametrize("c", (1, 8))
def test_real_valued_scatter_is_deterministic(c):
    """Segments of 200 real-valued entries: with integers any order of the sum gives the same bits, here only the
    fixed order does.  The order k_csr_fill's atomics ran in must not reach the sums: two builds agree in bits, and so
    do the built-per-call and the kept plan.  Against float64 the bound of tests/test_gpu_ski.py holds."""
    name = "clustered-N200"
    idx, _ = E.interp_case(name)
    B, M, N, J = E.case_shape(name)
    r = E.rng(6, c)
    vals = (0.2 + r.random((B, N, J))).astype(np.float32) / J
    v = r.standard_normal((B, N, c)).astype(np.float32)
    with profiled({"ski_csr_build", "ski_interp_t"}):
        g = Bands()
        runs = [interp_t(g, idx, vals, v, M) for _ in range(2)]
        runs += [interp_t_planned(g, K.interp_plan_build(dev(idx), M), vals, v, M) for _ in range(2)]
        assert g.intact()
    for other in runs[1:]:
        assert torch.equal(bits(runs[0]), bits(other))
    err = col_err(host(runs[0]), E.wt_ref(idx, vals, v, M))
    print(f"real-valued W^T v, c = {c}: column error {err:.3e}")
    assert err <= 2e-5
    assert not host(runs[0])[E.segment_lengths(idx, M) == 0].any()   # a point without entries is an exact 0
