"""Fixed-step iterates of `minres_solve` (csrc/lo_minres.hip), `minres_solve_f64` (csrc/lo_minres_f64.hip) and the
wrapper `utils.minres` against the oracle's float64 run: the case table, the references, the checker and the bounds are
tests/minres_cases.py (8 x what the oracle's own float32 run shows on the same inputs, between 2e-6 and 5e-4; 1e-10 for
the float64 engine; tests/test_minres_cases_cpu.py shows that every iterate compared still moves by 100 x its bound per
step and that the checker fails on what a wrong kernel would write).  Each test is one solver call on tiny operands
with `tolerance = 0` and `max_iter = k - 2`, i.e. exactly k iterations; the step count, `info.matvecs`, `info.converged`,
`info.conv` and the launch counts of k_mr_lanczos, k_mr_update and the shared k_dot_part epilogue are asserted with it.

Which case reaches what (values checked in every one of them):
  k_mr_norm, k_mr_init_scal, k_mr_lanczos, k_mr_givens, k_mr_update, k_mr_final over S = 2 and 4 slices with a short
      last slice            slices-N517-*, slices-N1027-*, slices-N1030-* (S = 1: N = 3, 6, 255, 260)
  k_mr_update's partial norms and k_mr_conv over S = 2 slices   slices-N517-k10 / -k11, stop-*, rhs-zero-column-tol1
  the thread map at nrs = 256, 128, 64, 51, 4, 3, 2, 2, 1, 1, 1   columns-c1 .. c256 (c = 257: refused)
  dot_part of another length than S    operand-dense-* (9, 33, 7, 9 partials), operand-kron-128x128 (1 against S = 64)
  the shared k_dot_part epilogue       operand-kron-3x5, -toeplitz, -sum, -closure*, precond-diag-*
  the Woodbury kernels' partials at S = 2 and 4   precond-woodbury-*
  lo_minres_f64                        f64-*

Measured on an MI355X: case, S, then for the relative error to the float64 oracle and for the difference of the
relative residuals the kernels' figure / the float32 oracle's / the bound, and the worst figure over its bound.  No
case is over its bound; the worst is 0.30 (slices-N6-k6).  The kernels mostly sit BELOW the float32 oracle's own
figure (they sum in slices and trees, numpy in one long chain), so most bounds are 10 - 50 x above what the kernels
show (worst ratio under 0.1 in 52 of the 62 float32 rows): loose by the 8 x rule, left as the rule sets them.  info.conv
was off by at most 5.1e-7 relative (bound 1e-5 .. 2.8e-5); float64: at most 2.5e-15 / 7.8e-16 against 1e-10.
  slices-N3-k2                 S=1   err 3.7e-07/3.6e-07/2.9e-06  resid 5.0e-08/9.6e-08/2.0e-06  worst 0.130
  slices-N3-k3                 S=1   err 1.6e-07/2.5e-07/2.0e-06  resid 2.9e-07/3.3e-07/2.6e-06  worst 0.110
  slices-N6-k2                 S=1   err 1.2e-07/1.9e-07/2.0e-06  resid 3.9e-08/4.6e-08/2.0e-06  worst 0.059
  slices-N6-k3                 S=1   err 1.6e-07/1.9e-07/2.0e-06  resid 3.0e-08/5.6e-08/2.0e-06  worst 0.080
  slices-N255-k2               S=1   err 1.6e-07/8.7e-07/6.9e-06  resid 1.9e-07/4.9e-07/4.0e-06  worst 0.049
  slices-N255-k3               S=1   err 2.3e-07/1.7e-06/1.4e-05  resid 1.4e-07/3.9e-07/3.1e-06  worst 0.045
  slices-N260-k2               S=1   err 2.5e-07/1.0e-06/8.3e-06  resid 1.0e-07/2.1e-07/2.0e-06  worst 0.050
  slices-N260-k3               S=1   err 3.0e-07/2.0e-06/1.6e-05  resid 1.2e-07/2.3e-07/2.0e-06  worst 0.058
  slices-N517-k2               S=2   err 1.7e-07/1.1e-06/8.5e-06  resid 3.1e-07/8.8e-07/7.1e-06  worst 0.044
  slices-N517-k3               S=2   err 4.5e-07/1.3e-06/1.0e-05  resid 3.8e-07/3.5e-07/2.8e-06  worst 0.135
  slices-N1027-k2              S=4   err 2.3e-07/3.5e-06/2.8e-05  resid 4.1e-07/6.0e-07/4.8e-06  worst 0.084
  slices-N1027-k3              S=4   err 3.3e-07/1.4e-06/1.1e-05  resid 1.5e-07/1.4e-06/1.1e-05  worst 0.030
  slices-N1030-k2              S=4   err 3.6e-07/1.2e-06/9.5e-06  resid 2.9e-07/1.3e-06/1.1e-05  worst 0.038
  slices-N1030-k3              S=4   err 6.5e-07/1.6e-06/1.3e-05  resid 2.0e-07/3.1e-06/2.5e-05  worst 0.050
  slices-N6-k6                 S=1   err 1.9e-06/1.2e-06/9.6e-06  resid 3.4e-05/1.4e-05/1.1e-04  worst 0.303
  slices-N517-k9               S=2   err 4.4e-07/8.7e-07/7.0e-06  resid 1.7e-08/2.1e-08/2.0e-06  worst 0.064
  slices-N517-k10              S=2   err 4.6e-07/8.7e-07/7.0e-06  resid 2.9e-08/2.5e-08/2.0e-06  worst 0.065
  slices-N517-k11              S=2   err 5.8e-07/1.1e-06/9.1e-06  resid 4.0e-08/4.4e-08/2.0e-06  worst 0.064
  columns-c1                   S=2   err 1.9e-07/6.3e-07/5.0e-06  resid 1.2e-07/3.6e-07/2.9e-06  worst 0.042
  columns-c2                   S=2   err 2.4e-07/1.7e-06/1.3e-05  resid 7.9e-08/1.8e-07/2.0e-06  worst 0.039
  columns-c4                   S=2   err 2.8e-07/1.2e-06/9.9e-06  resid 1.3e-07/3.8e-07/3.0e-06  worst 0.042
  columns-c5                   S=2   err 5.1e-07/2.6e-06/2.1e-05  resid 1.4e-07/3.5e-07/2.8e-06  worst 0.052
  columns-c64                  S=2   err 9.5e-07/4.0e-06/3.2e-05  resid 3.1e-07/2.2e-06/1.8e-05  worst 0.030
  columns-c85                  S=2   err 1.1e-06/3.4e-06/2.7e-05  resid 1.7e-07/1.0e-06/8.0e-06  worst 0.040
  columns-c86                  S=2   err 9.2e-07/3.8e-06/3.0e-05  resid 4.5e-07/2.1e-06/1.7e-05  worst 0.030
  columns-c128                 S=2   err 7.5e-07/4.0e-06/3.2e-05  resid 2.6e-07/1.4e-06/1.1e-05  worst 0.023
  columns-c129                 S=2   err 1.4e-06/3.2e-06/2.5e-05  resid 2.7e-07/1.5e-06/1.2e-05  worst 0.055
  columns-c255                 S=2   err 2.0e-06/3.7e-06/2.9e-05  resid 4.7e-07/1.1e-06/8.9e-06  worst 0.067
  columns-c256                 S=2   err 1.8e-06/3.5e-06/2.8e-05  resid 2.7e-07/9.3e-07/7.4e-06  worst 0.066
  shifts-Q1-shared             S=2   err 2.6e-07/9.0e-07/7.2e-06  resid 7.4e-08/9.3e-07/7.4e-06  worst 0.036
  shifts-Q1-member             S=2   err 3.3e-07/1.1e-06/8.7e-06  resid 3.4e-08/3.7e-07/2.9e-06  worst 0.038
  shifts-Q5-member-B3          S=2   err 5.8e-07/1.0e-06/8.0e-06  resid 1.1e-07/8.0e-07/6.4e-06  worst 0.072
  shifts-Q15-shared            S=2   err 4.0e-07/1.2e-06/1.0e-05  resid 2.1e-07/9.5e-07/7.6e-06  worst 0.041
  shifts-value-1               S=2   err 2.8e-07/1.7e-06/1.4e-05  resid 2.8e-09/2.5e-08/2.0e-06  worst 0.020
  shifts-value2.5              S=2   err 1.5e-07/1.2e-06/9.7e-06  resid 1.4e-07/5.1e-07/4.1e-06  worst 0.034
  shifts-indefinite            S=2   err 5.9e-07/1.7e-06/1.3e-05  resid 7.7e-09/1.8e-08/2.0e-06  worst 0.044
  rhs-scales                   S=2   err 2.0e-07/2.7e-06/2.1e-05  resid 5.0e-08/6.5e-07/5.2e-06  worst 0.010
  rhs-zero-column              S=2   err 2.4e-07/1.7e-06/1.3e-05  resid 1.6e-07/4.5e-07/3.6e-06  worst 0.045
  rhs-zero-column-tol1         S=2   err 5.7e-07/6.3e-07/5.1e-06  resid 2.5e-08/2.5e-08/2.0e-06  worst 0.113
  operand-dense-mfma           S=2   err 5.3e-07/1.3e-06/1.0e-05  resid 1.1e-07/1.5e-07/2.0e-06  worst 0.054
  operand-dense-valu16         S=2   err 1.6e-07/1.6e-07/2.0e-06  resid 2.8e-08/1.8e-08/2.0e-06  worst 0.079
  operand-dense-small          S=1   err 2.1e-07/4.4e-07/3.5e-06  resid 4.1e-08/9.7e-08/2.0e-06  worst 0.059
  operand-dense-valu32         S=1   err 6.1e-07/7.2e-07/5.8e-06  resid 2.1e-07/1.6e-07/2.0e-06  worst 0.105
  operand-kron-3x5             S=1   err 1.2e-07/1.2e-07/2.0e-06  resid 3.4e-08/5.4e-08/2.0e-06  worst 0.061
  operand-kron-128x128         S=64  err 1.7e-07/1.6e-07/2.0e-06  resid 3.7e-09/2.6e-09/2.0e-06  worst 0.086
  operand-toeplitz             S=2   err 3.6e-07/9.3e-07/7.4e-06  resid 1.4e-08/1.8e-08/2.0e-06  worst 0.048
  operand-sum                  S=2   err 4.9e-07/1.9e-06/1.5e-05  resid 3.6e-07/3.3e-07/2.6e-06  worst 0.137
  operand-closure              S=2   err 5.0e-07/8.0e-07/6.4e-06  resid 2.0e-07/9.7e-07/7.8e-06  worst 0.079
  operand-closure-c1           S=2   err 3.0e-07/2.5e-07/2.0e-06  resid 2.1e-07/1.2e-07/2.0e-06  worst 0.151
  operand-tensor               S=2   err 4.0e-07/1.6e-06/1.3e-05  resid 6.5e-08/1.3e-07/2.0e-06  worst 0.032
  precond-woodbury-r1-N517     S=2   err 2.2e-07/1.9e-06/1.6e-05  resid 2.1e-07/1.1e-06/9.0e-06  worst 0.023
  precond-woodbury-r5-N1030    S=4   err 2.9e-07/1.0e-06/8.3e-06  resid 1.9e-07/4.0e-07/3.2e-06  worst 0.058
  precond-woodbury-r8-N517     S=2   err 2.6e-07/1.3e-06/1.0e-05  resid 1.2e-07/6.3e-07/5.1e-06  worst 0.025
  precond-woodbury-r8-N1030    S=4   err 3.5e-07/3.1e-07/2.5e-06  resid 1.8e-08/5.2e-08/2.0e-06  worst 0.144
  precond-diag-N517            S=2   err 3.0e-07/1.2e-06/9.3e-06  resid 8.7e-08/4.0e-07/3.2e-06  worst 0.033
  precond-diag-N1030           S=4   err 3.0e-07/1.6e-06/1.3e-05  resid 1.4e-07/5.6e-07/4.5e-06  worst 0.032
  stop-at-10                   S=2   err 5.3e-07/7.2e-07/5.8e-06  resid 1.3e-08/1.9e-08/2.0e-06  worst 0.091
  stop-at-20                   S=2   err 5.5e-07/6.4e-07/5.1e-06  resid 2.3e-08/1.4e-08/2.0e-06  worst 0.107
  stop-runs-out                S=2   err 5.3e-07/9.9e-07/7.9e-06  resid 2.8e-08/2.8e-08/2.0e-06  worst 0.067
  stop-max-iter-0              S=2   err 2.3e-07/1.1e-06/8.9e-06  resid 5.8e-08/5.9e-07/4.7e-06  worst 0.026
  wrapper-cap-N6               S=1   err 1.5e-07/1.9e-07/2.0e-06  resid 1.7e-07/2.2e-07/2.0e-06  worst 0.086
  wrapper-broadcast            S=2   err 2.5e-07/2.0e-06/1.6e-05  resid 1.3e-07/4.3e-07/3.4e-06  worst 0.038
  f64-dense-B1-N3-c1 2.0e-16 / 1.1e-16, -B3-N64-c3 8.8e-16 / 1.7e-16, -B1-N257-c7 2.5e-15 / 6.7e-16, -B3-N517-c3-member
  1.7e-15 / 4.4e-16, -value-1 3.6e-16 / 4.2e-17, -zero-column 7.6e-16 / 1.4e-16, -stop-at-10 2.2e-15 / 8.7e-17,
  f64-closure 1.5e-15 / 2.5e-16, -lowrank-desc 2.1e-15 / 7.8e-16, -kron-desc 4.7e-16 / 2.5e-16, -precond-pair
  2.2e-15 / 3.9e-16, -precond-closure 2.1e-15 / 3.3e-16   (err / resid, bound 1e-10 each)"""
import numpy as np
import pytest
import torch

import minres_cases as mc

pytestmark = pytest.mark.gpu

from linear_operator_amd import _hip, kernels as K, settings  # noqa: E402

f64 = np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def profiled(fn):
    """(fn(), {kernel class: (launches, ms)}) of one call."""
    K._hip.prof_enable(True)
    try:
        K._hip.prof_report()
        out = fn()
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
    finally:
        K._hip.prof_enable(False)
    return out, prof


def descriptor(c, o):
    """The float32 descriptor of a case (None: the operator is a closure)."""
    d = dev(o["d"])
    if c.kind == "lowrank":
        return K.lowrank_diag_descriptor(dev(o["C"]), d)
    if c.kind == "dense":
        return K.dense_diag_descriptor(dev(o["K"]), d)
    if c.kind == "kron":
        return K.kron_diag_descriptor(dev(o["K1"]), dev(o["K2"]), d)
    if c.kind == "toeplitz":
        return K.toeplitz_diag_descriptor(dev(o["col"]), d)
    if c.kind == "sum":
        return K.sum_descriptor([K.lowrank_diag_descriptor(dev(o["C"]), None), K.dense_diag_descriptor(dev(o["K"]), None)], d)
    assert c.kind == "closure", c.kind
    return None


def through_the_wrapper(c, o, monkeypatch):
    """The MinresResult of the K.minres_solve call that utils.minres makes for a wrapper or a dense-tensor case."""
    from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, LowRankRootLinearOperator
    from linear_operator_amd.utils import minres

    seen = []

    def recording(*a, _real=K.minres_solve, **kw):
        seen.append(_real(*a, **kw))
        return seen[-1]

    monkeypatch.setattr(K, "minres_solve", recording)
    rhs, sh = dev(o["rhs"]), dev(o["shifts"])
    if c.kind == "tensor":
        closure = dev(mc.dense_tensor(c.name))
    else:
        A = AddedDiagLinearOperator(LowRankRootLinearOperator(dev(o["C"])), DiagLinearOperator(dev(o["d"])))
        closure = A._matmul
        if c.opts["wrapper"] == "broadcast":
            rhs = rhs[0]
    with settings.minres_tolerance(c.tol):
        x = minres(closure, rhs, shifts=sh, value=c.value, max_iter=c.max_iter)
    assert len(seen) == 1 and tuple(x.shape) == (c.Q, c.B, c.N, c.c) and torch.equal(x, seen[0].x.reshape(x.shape))
    return seen[0]


def run_f32(c, monkeypatch):
    o = mc.operands(c.name)
    if c.kind == "tensor" or "wrapper" in c.opts:
        return profiled(lambda: through_the_wrapper(c, o, monkeypatch))
    desc, closure, kw = descriptor(c, o), None, {}
    if desc is None:
        Ct, dt = dev(o["C"]), dev(o["d"])
        closure = lambda v: Ct @ (Ct.mT @ v) + dt.unsqueeze(-1) * v  # noqa: E731
    if isinstance(c.precond, tuple):
        kw["precond"] = K.precond_build(dev(o["L"]), dev(o["pd"]), False)
    elif c.precond == "diag":
        p = dev(o["p"]).unsqueeze(-1)
        kw["precond_closure"] = lambda v: v / p
    rhs, sh = dev(o["rhs"]), dev(o["shifts"])
    torch.cuda.synchronize()
    return profiled(lambda: K.minres_solve(desc, rhs, sh, value=c.value, matvec_closure=closure, max_iter=c.max_iter,
                                           tolerance=c.tol, **kw))


def run_f64(c):
    o = mc.operands(c.name)
    A, kw = None, {}
    if c.kind in ("f64dense", "f64closure"):
        full = dev(o["K"] + np.stack([np.diag(x) for x in o["d"]]))
        if c.kind == "f64dense":
            A = full
        else:
            kw["matvec_closure"] = lambda v: full @ v
    elif c.kind == "f64lowrank":
        kw["desc"] = K.lowrank_diag_descriptor(dev(o["C"]), dev(o["d"]), dtype=torch.float64)
    else:
        kw["desc"] = K.kron_diag_descriptor(dev(o["K1"]), dev(o["K2"]), dev(o["d"]), dtype=torch.float64)
    if isinstance(c.precond, tuple):
        Q, noise = mc.woodbury_pair64(c.name)
        kw["precond"] = (dev(Q), dev(noise), False)
    elif c.precond == "diag":
        p = dev(o["p"]).unsqueeze(-1)
        kw["precond_closure"] = lambda v: v / p
    return K.minres_solve_f64(A, dev(o["rhs"]), dev(o["shifts"]), value=c.value, max_iter=c.max_iter, tolerance=c.tol, **kw)


def assert_result(c, res, matvecs):
    """Shape, counts, stop state and the checker's figures of one run against the float64 oracle's."""
    _, info, conv = mc.reference(c.name)
    assert tuple(res.x.shape) == (c.Q, c.B, c.N, c.c), (c.name, res.x.shape)
    assert res.x.dtype == (torch.float32 if c.dtype == "f32" else torch.float64)
    assert res.iterations == c.k == info.iterations, (c.name, res.iterations, info.iterations)
    assert res.matvecs == matvecs, (c.name, res.matvecs)
    assert res.converged == info.converged, (c.name, res.converged, res.conv)
    vals, bnd = mc.check(c.name, host(res.x)), mc.bounds(c.name)
    line = mc.tag(c.name, vals, bnd)
    if conv:  # the last check the run made
        at = max(conv)
        if np.isnan(conv[at]):
            assert np.isnan(res.conv), (c.name, res.conv)
        else:
            rel, cb = abs(res.conv - conv[at]) / conv[at], mc.conv_bound(c.name, at)
            line += f"  conv {res.conv:.4e} (oracle {conv[at]:.4e}, off {rel:.1e}, bound {cb:.1e})"
            assert rel <= cb, line
    else:
        assert res.conv == 0.0, (c.name, res.conv)
    print(line)
    assert not mc.violations(vals, bnd), (mc.violations(vals, bnd), line)


@pytest.mark.parametrize("name", mc.F32_CASES)
def test_float32_iterate_against_the_float64_oracle(name, monkeypatch):
    c = mc.BY_NAME[name]
    res, prof = run_f32(c, monkeypatch)
    launches = {k: prof.get(k, (0, 0.0))[0] for k in ("mr_lanczos", "mr_update", "vec_dot_part")}
    assert launches == dict(mr_lanczos=c.k, mr_update=c.k, vec_dot_part=mc.expected_vec_dot_part(c)), (name, launches)
    assert_result(c, res, matvecs=c.k)


@pytest.mark.parametrize("name", mc.F64_CASES)
def test_float64_iterate_against_the_float64_oracle(name):
    c = mc.BY_NAME[name]
    assert_result(c, run_f64(c), matvecs=c.k + 1)  # (one product more: the reference's shape probe, :66-68)


@pytest.mark.parametrize("name", mc.REFUSED)
def test_refusals_launch_nothing(name):
    """One iteration (max_iter = -1) and 257 columns in float32, Q B > 65535 in float64: the unsupported error, before
    any launch."""
    c, o = mc.BY_NAME[name], mc.operands(name)
    rhs, sh = dev(o["rhs"]), dev(o["shifts"])
    if c.dtype == "f32":
        desc = K.lowrank_diag_descriptor(dev(o["C"]), dev(o["d"]))
        call = lambda: K.minres_solve(desc, rhs, sh, max_iter=c.max_iter, tolerance=0.0)  # noqa: E731
    else:
        A = dev(o["K"] + np.stack([np.diag(x) for x in o["d"]]))
        call = lambda: K.minres_solve_f64(A, rhs, sh, max_iter=c.max_iter, tolerance=0.0)  # noqa: E731
    assert (c.max_iter == -1) == (c.opts["refused"] == "iterations") and (c.c > mc.MAX_COLS) == (c.opts["refused"] == "columns")
    torch.cuda.synchronize()

    def refused():
        with pytest.raises(_hip.HipExtensionError, match="unsupported shape"):
            call()

    _, prof = profiled(refused)
    assert prof == {}, (name, prof)
