"""Every step route of `lanczos_tridiag` (csrc/lo_lanczos.hip), `lanczos_tridiag_f64` (csrc/lo_lanczos_f64.hip) and the
root epilogue against the recurrence itself, in float64: the case table, the checker and the bounds are
tests/lanczos_cases.py (8 x what the oracle's own run in the same precision shows on the same inputs, capped at 1e-4 /
1e-10; tests/test_lanczos_invariants_cpu.py shows that the checker fails on what a wrong kernel would write).  Each
test is one call on tiny operands; the route that ran is read from the launch profile.

Which case reaches which kernel (values checked in every one of them):
  k_lz_alpha, k_lz_dots_fused<20>, k_lz_reduce_pred, k_lz_correct_check<20>, k_lz_finish   fused-*, dense-*, closure-*,
      stop-fused-P4, global-stop-P4 (fused-N260-P4-k2 and the last step of every fused case: k_lz_alpha alone)
  k_lz_sub_prev_dot, k_lz_multidot4<24>, k_lz_correct4<24>   plain4-*, unfused-*, stop-plain4-P4
  k_lz_multidot<24>, k_lz_correct<24>                         scalar-*, stop-scalar-P3
  k_lz_multidot_any, k_lz_correct_any                         plain4-N300-P8-k26 (from step 24 on), scalar-N64-P3-k30
  k_lz_dot, k_lz_scal, k_lz_axpy                              every case (single-* runs nothing else)
  k_lz_permute                                                test_contiguous_copy_equals_the_view
  k_lz_root<16>, <32>, k_lz_root_native<16>, <32>             test_root_epilogue_*

Measured on an MI355X, kernels / oracle's float32 run (the bound is 8 x the second figure): case, route the profile
showed, vectors returned, q0, orth, proj, resid and, where k = N, recon.  The worst value over bound was 0.25 in float32
and 0.47 in float64; the root epilogue reached at most 0.45 of its derived bound.
  fused-N517-P4-k21     fused  21  1.4e-08/6.9e-08  2.5e-07/1.1e-06  1.3e-07/6.7e-07  3.6e-08/1.5e-07
  fused-N260-P8-k20     fused  20  1.3e-08/3.5e-08  1.9e-07/5.8e-07  8.2e-08/5.4e-07  3.9e-08/2.1e-07
  fused-N260-P32-k20    fused  20  1.8e-08/5.5e-08  2.4e-07/8.5e-07  1.6e-07/6.1e-07  5.1e-08/1.8e-07
  fused-N260-P64-k20    fused  20  2.9e-08/4.8e-08  3.1e-07/9.2e-07  1.0e-07/7.3e-07  4.5e-08/2.4e-07
  fused-N1030-P16-k7    fused   7  1.5e-08/4.5e-08  2.3e-07/1.5e-06  1.4e-07/1.1e-06  3.0e-08/1.8e-07
  fused-N6-P4-k9        fused   6  4.4e-08/4.4e-08  3.6e-07/2.5e-07  2.0e-07/1.6e-07  9.1e-08/6.2e-08  1.2e-07/1.0e-07
  fused-N260-P4-k2      alpha   2  1.9e-08/2.2e-08  1.3e-07/2.1e-07  3.3e-08/6.6e-07  3.4e-09/1.0e-08
  dense-N517-P4-k12     fused  12  9.8e-09/5.4e-08  1.9e-07/1.0e-06  1.5e-07/6.0e-07  8.1e-08/1.4e-07
  closure-N517-P4-k12   fused  12  1.5e-08/4.2e-08  1.8e-07/1.1e-06  1.4e-07/7.7e-07  3.2e-08/2.0e-07
  plain4-N517-P4-k22    plain  22  8.4e-09/4.6e-08  1.7e-07/8.9e-07  8.1e-08/6.7e-07  3.8e-08/1.6e-07
  plain4-N300-P8-k26    plain  26  1.3e-08/4.4e-08  2.0e-07/9.0e-07  7.1e-08/4.6e-07  3.8e-08/1.4e-07
  plain4-N40-P4-k40     plain  40  2.8e-08/5.9e-08  2.1e-07/3.7e-07  9.0e-08/1.6e-07  6.7e-08/1.0e-07  3.7e-08/7.1e-08
  unfused-N517-P4-k21   plain  21  1.2e-08/3.4e-08  1.9e-07/8.1e-07  1.2e-07/6.6e-07  3.9e-08/2.2e-07
  unfused-N260-P64-k20  plain  20  2.2e-08/4.8e-08  2.5e-07/8.2e-07  1.5e-07/7.3e-07  6.0e-08/2.2e-07
  scalar-N517-P1-k12    plain  12  1.4e-08/2.0e-08  1.6e-07/1.7e-07  6.2e-08/1.1e-07  2.8e-08/4.2e-08
  scalar-N517-P2-k12    plain  12  1.2e-08/1.2e-08  1.3e-07/8.4e-07  1.4e-07/8.1e-07  2.8e-08/1.4e-07
  scalar-N517-P3-k12    plain  12  1.2e-08/4.2e-08  1.9e-07/7.8e-07  8.6e-08/7.0e-07  3.4e-08/1.2e-07
  scalar-N517-P5-k12    plain  12  1.5e-08/3.8e-08  1.9e-07/8.9e-07  8.2e-08/6.2e-07  3.3e-08/1.2e-07
  scalar-N517-P17-k12   plain  12  1.5e-08/5.3e-08  1.8e-07/1.1e-06  1.2e-07/9.2e-07  3.6e-08/2.2e-07
  scalar-N64-P100-k6    plain   6  5.9e-08/5.8e-08  3.2e-07/4.0e-07  1.6e-07/3.4e-07  1.0e-07/1.4e-07
  scalar-N64-P128-k6    plain   6  4.5e-08/7.7e-08  3.0e-07/4.3e-07  1.5e-07/2.7e-07  8.2e-08/1.3e-07
  scalar-N64-P200-k6    plain   6  5.5e-08/5.6e-08  4.5e-07/5.1e-07  2.9e-07/4.2e-07  1.6e-07/1.6e-07
  scalar-N64-P256-k6    plain   6  6.7e-08/1.1e-07  4.8e-07/5.3e-07  3.3e-07/3.4e-07  1.6e-07/1.7e-07
  scalar-N64-P3-k30     plain  30  2.4e-08/2.4e-08  1.4e-07/2.9e-07  5.8e-08/2.2e-07  4.9e-08/9.7e-08
  scalar-N3-P1-k5       plain   3  1.2e-08/1.2e-08  1.8e-07/1.2e-07  1.6e-07/7.7e-08  6.5e-08/8.0e-08  1.4e-07/1.2e-07
  single-N517-P3-k1     none    1  1.3e-08/4.1e-08  8.6e-08/5.6e-07  4.3e-09/1.9e-08  0.0e+00/0.0e+00
  single-N517-P4-k1     none    1  9.1e-09/3.4e-08  1.2e-07/4.8e-07  1.9e-09/1.5e-08  0.0e+00/0.0e+00
  stop-fused-P4         fused   2  1.2e-08/4.3e-08  1.2e-07/4.6e-07  8.5e-08/2.5e-07  3.6e-09/3.6e-09
  stop-plain4-P4        plain   2  1.5e-08/3.6e-08  2.0e-07/4.1e-07  9.4e-08/5.9e-07  1.5e-09/1.6e-09
  stop-scalar-P3        plain   2  1.3e-08/6.0e-08  1.1e-07/6.6e-07  8.2e-08/2.0e-07  1.3e-09/4.2e-09
  global-stop-P4        fused  10  2.1e-08/3.6e-08  1.6e-07/6.7e-07  6.1e-08/4.4e-07  2.6e-08/1.0e-07"""
import numpy as np
import pytest
import torch

import lanczos_cases as lc

pytestmark = pytest.mark.gpu

from linear_operator_amd import kernels as K  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def profiled(fn):
    """(fn(), {kernel class: (launches, ms)}) of one call."""
    K._hip.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
    finally:
        K._hip.prof_enable(False)
    return out, prof


def route_of(prof):
    """The step route a launch profile shows."""
    fused, alpha, plain = "lz_dots_fused" in prof, "lz_alpha" in prof, "lz_sub_prev_dot" in prof
    assert not (plain and (fused or alpha)) and not (fused and not alpha), sorted(prof)
    return "fused" if fused else ("alpha" if alpha else ("plain" if plain else "none"))


def run_case(c):
    """(q, t, launch profile) of the case on the device."""
    o = lc.operands(c.name)
    V = dev(o["V"])
    closure = None
    if c.kind == "dense":
        desc = K.dense_diag_descriptor(dev(o["K"]), dev(o["d"]))
    elif c.kind == "closure":
        Ct, dt = dev(o["C"]), dev(o["d"])
        desc, closure = None, (lambda v: Ct @ (Ct.mT @ v) + dt.unsqueeze(-1) * v)
    else:  # low-rank descriptor; the rank-one operator is one with R = 1 and NO diagonal
        desc = K.lowrank_diag_descriptor(dev(o["C"]), None if o["d"] is None else dev(o["d"]))
    (q, t), prof = profiled(lambda: K.lanczos_tridiag(desc, V, c.max_iter, matvec_closure=closure))
    return q, t, prof


def assert_case(c, q, t, prof):
    qo, to = lc.oracle_run(c.name, "f32")
    k = t.shape[-1]
    lead = (() if c.P == 1 else (c.P,)) + (c.B,)
    assert tuple(q.shape) == lead + (c.N, k) and tuple(t.shape) == lead + (k, k), (c.name, q.shape, t.shape)
    if c.steps > 0:  # the step count and the shapes of the oracle's run
        assert k == c.steps and tuple(q.shape) == qo.shape and tuple(t.shape) == to.shape, (c.name, k, qo.shape)
    want = {"plain4": "plain", "scalar": "plain"}.get(c.route, c.route)
    assert route_of(prof) == want, (c.name, c.route, sorted(prof))
    vals, ref, bnd = lc.check_case(c.name, host(q), host(t)), lc.oracle_values(c.name, "f32"), lc.bounds(c.name)
    line = lc.tag(c.name, vals, ref, bnd)
    print(f"[{route_of(prof)} k={k}] {line}")
    assert ("recon" in vals) == (k == c.N), line
    assert not lc.violations(vals, bnd), (lc.violations(vals, bnd), line)


REGULAR = [c.name for c in lc.CASES if c.kind in ("lowrank", "dense", "closure")]


@pytest.mark.parametrize("name", REGULAR)
def test_route_against_the_recurrence(name, monkeypatch):
    c = lc.BY_NAME[name]
    if c.unfused:
        monkeypatch.setenv("LO_LZ_UNFUSED", "1")
    else:
        monkeypatch.delenv("LO_LZ_UNFUSED", raising=False)
    assert_case(c, *run_case(c))


@pytest.mark.parametrize("name", [c.name for c in lc.STOP_CASES])
def test_early_stop_after_the_krylov_space_is_exhausted(name, monkeypatch):
    """u u^T (a low-rank descriptor with R = 1 and no diagonal): the Krylov space has dimension 2, beta_1 is rounding
    noise for every probe and the run returns two vectors, on every route."""
    c = lc.BY_NAME[name]
    if c.unfused:
        monkeypatch.setenv("LO_LZ_UNFUSED", "1")
    else:
        monkeypatch.delenv("LO_LZ_UNFUSED", raising=False)
    q, t, prof = run_case(c)
    assert t.shape[-1] == 2, (name, t.shape)
    assert_case(c, q, t, prof)


def test_stop_flag_is_batch_global(monkeypatch):
    """Member 0 is exhausted after two vectors (its beta_1 is about 7e-8), member 1 is not: the run goes on.  A
    per-member stop flag, or one that keeps the last writer's value, would stop at step 1.  What member 0 holds after its
    exhaustion is noise (whether it can be re-orthogonalised is not pinned): it must be finite; member 1 must satisfy
    every invariant over the vectors returned."""
    monkeypatch.delenv("LO_LZ_UNFUSED", raising=False)
    c = lc.GLOBAL_STOP
    q, t, prof = run_case(c)
    assert t.shape[-1] >= 3, t.shape
    assert bool(torch.isfinite(q[:, 0]).all()) and bool(torch.isfinite(t[:, 0]).all())
    assert_case(c, q, t, prof)


# ---- float64 -----------------------------------------------------------------------------------------------------------
def assert_f64(shape, what, q, t, rank1=False):
    (qo, to), ref = lc.f64_oracle(*shape, rank1=rank1)
    assert q.dtype == torch.float64 and tuple(q.shape) == qo.shape and tuple(t.shape) == to.shape, (shape, what, q.shape)
    vals, bnd = lc.f64_check(*shape, host(q), host(t), rank1), lc.bounds_from(ref, "f64")
    line = lc.tag(f"f64 {shape} {what}", vals, ref, bnd)
    print(line)
    assert not lc.violations(vals, bnd), (lc.violations(vals, bnd), line)


@pytest.mark.parametrize("P,N,max_iter", lc.F64_SHAPES)
def test_float64_against_the_recurrence(P, N, max_iter):
    """Dense A + diag by the library's fp64 matvec, the same operator as a closure, and (one shape) as a float64
    low-rank descriptor."""
    shape = (P, N, max_iter)
    o = lc.f64_operands(*shape)
    At, dt, Vt = dev(o["A"]), dev(o["d"]), dev(o["V"])
    assert_f64(shape, "dense", *K.lanczos_tridiag_f64(At, dt, Vt, max_iter))
    assert_f64(shape, "closure", *K.lanczos_tridiag_f64(None, None, Vt, max_iter,
                                                        matvec_closure=lambda v: At @ v + dt.unsqueeze(-1) * v))
    if shape == lc.F64_DESC_SHAPE:
        desc = K.lowrank_diag_descriptor(dev(o["C"]), dt, dtype=torch.float64)
        assert_f64(shape, "desc", *K.lanczos_tridiag_f64(None, None, Vt, max_iter, desc=desc))


def test_float64_early_stop():
    P, N, max_iter = lc.F64_STOP
    o = lc.f64_operands(P, N, max_iter, True)
    q, t = K.lanczos_tridiag_f64(dev(o["A"]), None, dev(o["V"]), max_iter)
    assert t.shape[-1] == 2, t.shape
    assert_f64(lc.F64_STOP, "rank one", q, t, rank1=True)


# ---- root_from_lanczos and the layout copy -------------------------------------------------------------------------------
def root_outputs(shape, native):
    """The three outputs of root_from_lanczos on the synthetic inputs, q in the step kernels' layout (a permuted view of
    [k, B, N, P]) or contiguous, and the launch profile."""
    P, B, N, k = shape
    r = lc.root_inputs(shape)
    if native:
        q = torch.empty(k, B, N, P, dtype=torch.float32, device="cuda").permute(3, 1, 2, 0)
        q.copy_(dev(r["q"]))
        assert K._native_lanczos_layout(q) == (P, B)
    else:
        q = dev(r["q"])
        assert q.is_contiguous() and (k == 1 or K._native_lanczos_layout(q) is None)
    outs, prof = profiled(lambda: K.root_from_lanczos(q, dev(r["evecs"]), dev(r["evals"]), want_root=True,
                                                      want_inverse=True))
    return [host(x) for x in outs], prof


@pytest.mark.parametrize("native", [True, False], ids=["native", "contiguous"])
@pytest.mark.parametrize("shape", lc.ROOT_SHAPES, ids=str)
def test_root_epilogue_against_float64(shape, native):
    """Q V, Q V sqrt(lambda), Q V / sqrt(lambda) elementwise under the float32 dot-product bound, from both layouts
    (k_lz_root_native<16> / <32>, k_lz_root<16> / <32>).  (64, 1, 260, 20): the native entry reports unsupported (125 KB
    of LDS) and the call goes through the copy; the values must be the same."""
    outs, prof = root_outputs(shape, native)
    assert list(prof) == ["lz_root"] and prof["lz_root"][0] == 1, prof
    if native and shape in lc.ROOT_NATIVE_UNSUPPORTED:  # the entry itself says so (before it launches anything)
        P, B, N, k = shape
        r = lc.root_inputs(shape)
        q, v, e = dev(np.transpose(r["q"], (3, 1, 2, 0))), dev(r["evecs"]), dev(r["evals"])
        out = torch.empty(P * B, N, k, dtype=torch.float32, device="cuda")
        rc = K._hip.load().lo_root_from_lanczos_native_f32(K._hip.ptr(q), K._hip.ptr(v), K._hip.ptr(e), B, N, P, k,
                                                           K._hip.ptr(out), None, None, K._hip.stream_ptr(out.device))
        assert rc == K._hip.LO_ERR_UNSUPPORTED, rc
    worst = lc.root_err_over_bound(shape, outs)
    print(f"root {shape} {'native' if native else 'contiguous'}: err / bound = {worst:.3f}")
    assert worst <= 1.0, (shape, native, worst)


def test_root_epilogue_above_32_vectors_is_the_torch_expression():
    shape = lc.ROOT_TORCH_SHAPE
    outs, prof = root_outputs(shape, native=True)
    assert "lz_root" not in prof, prof
    worst = lc.root_err_over_bound(shape, outs)
    print(f"root {shape} torch: err / bound = {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("P,k,copies", [(4, 10, True), (3, 5, True), (64, 8, False)])
def test_contiguous_copy_equals_the_view(P, k, copies):
    """`contiguous=True`: P % 4 == 0 with k % 4 != 0 (no float4 copy) and P = 3 through k_lz_permute, P = 64 where the
    copy kernel reports unsupported (66.6 KB of LDS) and torch copies."""
    B, N = 2, 77
    C, d, _ = lc.cases.lowrank_diag(7700 + P, B, N, 4, 1)
    V = dev(lc.cases.randn(7701 + P, B, N, P, dtype=np.float32))
    desc = K.lowrank_diag_descriptor(dev(C), dev(d))
    q_view, t_view = K.lanczos_tridiag(desc, V, k)
    (q_cont, t_cont), prof = profiled(lambda: K.lanczos_tridiag(desc, V, k, contiguous=True))
    assert ("lz_permute" in prof) == copies, sorted(prof)
    assert tuple(q_cont.shape) == (P, B, N, k) and q_cont.is_contiguous() and not q_view.is_contiguous()
    assert torch.equal(q_view, q_cont) and torch.equal(t_view, t_cont)
