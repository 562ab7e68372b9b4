"""The matrix-free LMC operator sum_q Kron(Kernel_q(X, X), Dense(B_q)) on the MI355X: lo_kernel_lmc_mv_f32
(csrc/lo_kernel_lmc.hip) against the float64 dense composition, the kind LO_OP_KERNEL_LMC_DIAG through the public API
(product, solve, inv_quad_logdet, pivoted Cholesky, gradients) against the reference's goldens
(tests/golden/g46_kernel_lmc_*.npz), its error codes and refusals, its routing and its memory.

Bounds: the protocol of tests/test_gpu_kernel_kron.py.  Golden quantities: the error against the fixture's float64 value is
at most REF_FACTOR = 4 times the reference's own recorded float32 error (floored at ERR_FLOOR = 1e-7).  The direct entry
point: 4 times the error of the torch float32 dense composition (sum_q K_q (x) B_q formed densely, one matmul) on the same
inputs, same floor.  Gradients through inv_quad: 4 times the error of the float32 run of the same computation on the STORED
dense operator.  Every test prints the ratio it measured (DESIGN.md section 6t holds the table)."""
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_lmc import (  # noqa: E402
    CASES, ERR_FLOOR, PROBES, RANK, dense_kron, dense_lmc, grad_keys, grad_names, inputs, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

from linear_operator_amd import _hip, covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, SumKroneckerLinearOperator, SumLinearOperator)

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0}
LMC = _hip.LO_OP_KERNEL_LMC_DIAG


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def host(t):
    return t.detach().double().cpu().numpy()


def within(label, err, ref_err):
    ref_err = max(ref_err, ERR_FLOOR)
    print(f"kernel_lmc {label}: err {err:.3e} reference fp32 {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (label, err, ref_err)


def guarded(fn, n):
    """A covar_func of the same native family that fails on any dense evaluation: both arguments with all n points."""
    def covar(x1, x2, **params):
        if x1.shape[-2] >= n and x2.shape[-2] >= n:
            raise AssertionError(f"covar_func was evaluated densely: {tuple(x1.shape)} x {tuple(x2.shape)}")
        return fn(x1, x2, **params)

    covar.native_family = fn.native_family
    return covar


def make_inputs(seed, Q, B, n, D, T, c, kind="plain"):
    """Points, per term hyperparameters (ARD for the even terms, a shared lengthscale for the odd ones, the scales of the
    terms a factor apart) and a NON-symmetric B_q, columns and a full diagonal that differs per (i, t)."""
    g = rng(seed)
    x = g.random((B, n, D)).astype(np.float32)
    if kind == "dup":  # every other point repeats its neighbour: pairs with r = 0 off the diagonal
        x[:, 1::2] = x[:, : x[:, 1::2].shape[1] * 2: 2]
    if kind == "far":  # separations of thousands of lengthscales: every off-diagonal kernel value underflows to 0
        x = (x * 4000.0).astype(np.float32)
        x[:, :, 0] += 4000.0 * np.arange(n, dtype=np.float32)[None, :]
    ls = [(0.35 * np.sqrt(D) * (0.6 + 0.5 * q) * (0.7 + 0.6 * g.random((B, 1, D if q % 2 == 0 else 1)))).astype(np.float32)
          for q in range(Q)]
    os_ = [(0.6 + 0.5 * g.random(B)).astype(np.float32) for _ in range(Q)]
    Bt = (np.eye(T) * (1.0 + 0.3 * np.arange(T)) + 0.5 * (g.random((B, Q, T, T)) - 0.3) * (1 - np.eye(T))).astype(np.float32)
    v = g.standard_normal((B, n * T, c)).astype(np.float32)
    d = (0.05 + g.random((B, n * T))).astype(np.float32)
    return x, ls, os_, Bt, v, d


def composition(fns, x, ls, os_, Bt, v, d, diag, dtype):
    """(sum_q K_q (x) B_q) v + d o v with the operator stored densely, in `dtype` on the device."""
    tx = dev(x, dtype)
    A = sum(dense_kron(fn(tx, tx, dev(ls[q], dtype), dev(os_[q], dtype)), dev(Bt[:, q], dtype)) for q, fn in enumerate(fns))
    y = A @ dev(v, dtype)
    if diag == "full":
        y = y + dev(d, dtype)[:, :, None] * dev(v, dtype)
    elif diag == "const":
        y = y + dev(d[:, :1], dtype)[:, :, None] * dev(v, dtype)
    return y


def operands(fns, x, ls, os_, d, diag, order=None):
    B, n, D = x.shape
    order = list(range(len(fns))) if order is None else order
    theta = K.kernel_sum_theta([dev(ls[q]) for q in order], [dev(os_[q]) for q in order], (B,), D)
    fams = [fns[q].native_family for q in order]
    dd = None if diag == "none" else (dev(d) if diag == "full" else dev(d[:, 0]))
    return theta, fams, dd


def direct(fns, x, ls, os_, Bt, v, d, diag, order=None):
    theta, fams, dd = operands(fns, x, ls, os_, d, diag, order)
    task = dev(Bt if order is None else Bt[:, order])
    return K.kernel_lmc_mv(dev(x), theta, task, fams, dev(v), dd, const_diag=diag == "const")


# (families, B, n, D, T, c, diagonal): Q of {1, 2, 3, 4}, every family and mixtures, ARD and shared lengthscales that differ
# per term (make_inputs), every padded D (1, 3, 8, 16, 32), T of {1, 2, 3, 8}, wide columns T c of {1, 2, 4, 24, 51} (every
# accumulator width, several sweeps with a ragged tail; 24 and 51 at Q = 4 in sweeps of 8, 51 at Q = 2 in sweeps of 16),
# n of {1, 63, 130, 257, 300}: one tile / a ragged tile / several tiles / more than one row block, split (B 1 or 3) and
# unsplit (512 x 40) points, every diagonal mode
DIRECT_CASES = [
    (("rbf", "matern52"), 3, 257, 3, 2, 1, "full"),
    (("matern12",), 1, 63, 1, 1, 4, "const"),
    (("matern32", "rbf", "matern12", "matern52"), 1, 130, 32, 8, 3, "full"),
    (("matern52", "matern32"), 1, 300, 8, 3, 17, "none"),
    (("matern52", "matern32"), 1, 300, 8, 3, 17, "full"),
    (("rbf", "matern12", "matern32", "matern52"), 1, 300, 16, 3, 17, "const"),
    (("rbf", "rbf"), 512, 40, 2, 2, 2, "const"),
    (("rbf", "matern32"), 512, 40, 2, 2, 2, "full"),
    (("rbf",), 1, 1, 1, 1, 1, "none"),
    (("matern12", "matern52", "rbf"), 3, 257, 3, 2, 1, "none"),
]


def case_id(case):
    return "+".join(case[0]) + "-" + "-".join(str(a) for a in case[1:])


@pytest.mark.parametrize("case", DIRECT_CASES, ids=case_id)
def test_direct_entry_point_against_the_fp64_composition(case):
    names, B, n, D, T, c, diag = case
    Q = len(names)
    fns = [covariance.FAMILIES[name] for name in names]
    x, ls, os_, Bt, v, d = make_inputs(9600 + DIRECT_CASES.index(case), Q, B, n, D, T, c)
    if T > 1:
        for q in range(Q):
            assert not np.allclose(Bt[:, q], Bt[:, q].transpose(0, 2, 1))  # (a transposed task product would not pass)
    lib = _hip.load()
    assert (lib.lo_kernel_lmc_mv_workspace_bytes(B, n, D, Q, T, c) == 256) == (B == 512 or n <= 128)  # (one tile, or workgroups enough: no split)
    want = host(composition(fns, x, ls, os_, Bt, v, d, diag, torch.float64))
    comp = host(composition(fns, x, ls, os_, Bt, v, d, diag, torch.float32))
    y = direct(fns, x, ls, os_, Bt, v, d, diag)
    assert y.shape == (B, n * T, c) and torch.isfinite(y).all()
    within("mv " + case_id(case), rel(host(y), want), rel(comp, want))
    if Q > 1:  # the terms swapped together in theta, the families and Bt: the same operator
        order = list(range(Q))[::-1]
        within("mv permuted " + case_id(case), rel(host(direct(fns, x, ls, os_, Bt, v, d, diag, order)), want),
               rel(comp, want))
    # the kind through lo_matvec_f32 runs the same kernel: the same bits
    theta, fams, dd = operands(fns, x, ls, os_, d, diag)
    desc = K.kernel_lmc_diag_descriptor(dev(x), theta, fams, dev(Bt), dd, const_diag=diag == "const")
    assert desc.kind == LMC and desc.N == n * T and desc.kernel_terms == T and K.kernel_lmc_terms(desc) == Q
    assert desc.n2 & 0xffff == K.kernel_sum_pack_families(fams)
    assert torch.equal(K.matvec(desc, dev(v)), y)


@pytest.mark.parametrize("kind", ["dup", "far"])
def test_direct_entry_point_with_coincident_and_with_far_points(kind):
    names, B, n, D, T, c = ("matern12", "matern52"), 1, 130, 3, 3, 4
    fns = [covariance.FAMILIES[name] for name in names]
    x, ls, os_, Bt, v, d = make_inputs(9700, 2, B, n, D, T, c, kind=kind)
    assert not np.allclose(ls[0].mean(), ls[1].mean(), rtol=0.2)  # (the terms' lengthscales differ)
    want = host(composition(fns, x, ls, os_, Bt, v, d, "full", torch.float64))
    comp = host(composition(fns, x, ls, os_, Bt, v, d, "full", torch.float32))
    y = direct(fns, x, ls, os_, Bt, v, d, "full")
    assert torch.isfinite(y).all()
    within(f"mv {kind}", rel(host(y), want), rel(comp, want))
    if kind == "far":  # only the diagonal blocks survive: y[(i, t)] = sum_q os_q^2 sum_s B_q[t, s] v[(i, s)] + d o v
        v4 = v.reshape(B, n, T, c).astype(np.float64)
        blocks = sum(os_[q].astype(np.float64)[:, None, None, None] ** 2
                     * np.einsum("bts,bisc->bitc", Bt[:, q].astype(np.float64), v4) for q in range(2))
        assert rel(host(y), blocks.reshape(B, n * T, c) + d[:, :, None].astype(np.float64) * v) <= 1e-6


@pytest.mark.parametrize("shape", [(1, 300, 8, 3, 17), (512, 40, 2, 2, 2)], ids=["split", "unsplit"])
def test_two_calls_give_the_same_bits(shape):
    B, n, D, T, c = shape
    fns = [covariance.matern32, covariance.rbf, covariance.matern12]
    x, ls, os_, Bt, v, d = make_inputs(9800, 3, B, n, D, T, c)
    assert (_hip.load().lo_kernel_lmc_mv_workspace_bytes(B, n, D, 3, T, c) > 256) == (B == 1)
    assert torch.equal(direct(fns, x, ls, os_, Bt, v, d, "full"), direct(fns, x, ls, os_, Bt, v, d, "full"))


def test_error_codes_of_the_entry_point():
    lib, p = _hip.load(), _hip.ptr
    B, n, D, Q, T, c = 1, 300, 3, 2, 2, 2
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, Q, D + 1, device=DEV)
    Bt = torch.eye(T, device=DEV).expand(B, Q, T, T).contiguous()
    v = torch.randn(B, n * T, c, device=DEV)
    y = torch.full((B, n * T, c), -7.0, device=DEV)
    dfull = torch.ones(B, n * T, device=DEV)
    st = _hip.stream_ptr(v.device)
    need = lib.lo_kernel_lmc_mv_workspace_bytes(B, n, D, Q, T, c)
    assert need > 256  # (a split member: partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def mv(xx=x, th=theta, tk=Bt, fam=0x30, b=B, nn=n, dim=D, qq=Q, tt=T, vv=v, cc=c, dd=None, mode=0, yy=y, w=ws, wb=need):
        return lib.lo_kernel_lmc_mv_f32(p(xx), p(th), p(tk), fam, b, nn, dim, qq, tt, p(vv), cc, p(dd), mode, p(yy), p(w),
                                        wb, st)

    assert mv() == 0 and mv(dd=dfull, mode=1) == 0
    torch.cuda.synchronize()
    y.fill_(-7.0)
    for bad in (dict(xx=None), dict(th=None), dict(tk=None), dict(vv=None), dict(yy=None), dict(b=0), dict(nn=0),
                dict(nn=-1), dict(dim=0), dict(cc=0), dict(tt=0), dict(tt=-1), dict(qq=0), dict(qq=-1), dict(fam=0x04),
                dict(fam=0x40), dict(fam=-1), dict(fam=0x100), dict(fam=0x10000), dict(mode=1), dict(mode=2), dict(mode=3)):
        assert mv(**bad) == -1, bad  # LO_ERR_BADARG (0x100: a code set beyond the Q = 2 terms)
    wide, th33 = torch.rand(1, 10, 33, device=DEV), torch.ones(1, Q, 34, device=DEV)
    v20, y20 = torch.randn(1, 20, 1, device=DEV), torch.full((1, 20, 1), -7.0, device=DEV)
    assert mv(xx=wide, th=th33, nn=10, dim=33, vv=v20, cc=1, yy=y20) == _hip.LO_ERR_UNSUPPORTED
    B9 = torch.eye(9, device=DEV).expand(1, Q, 9, 9).contiguous()
    v90, y90 = torch.randn(1, 90, 1, device=DEV), torch.full((1, 90, 1), -7.0, device=DEV)
    assert mv(tk=B9, nn=10, tt=9, vv=v90, cc=1, yy=y90) == _hip.LO_ERR_UNSUPPORTED
    th5, B5 = torch.ones(1, 5, D + 1, device=DEV), torch.eye(T, device=DEV).expand(1, 5, T, T).contiguous()
    assert mv(th=th5, tk=B5, qq=5, fam=0) == _hip.LO_ERR_UNSUPPORTED
    assert mv(b=65536) == _hip.LO_ERR_UNSUPPORTED and mv(nn=0x7ffffe01) == _hip.LO_ERR_UNSUPPORTED  # (the 32-bit limits)
    assert mv(nn=0x40000000) == _hip.LO_ERR_UNSUPPORTED and mv(tt=8, cc=0x10000000) == _hip.LO_ERR_UNSUPPORTED
    for args in ((1, 10, 33, 2, 2, 1), (1, 10, 3, 2, 9, 1), (1, 10, 3, 5, 2, 1)):
        assert lib.lo_kernel_lmc_mv_workspace_bytes(*args) == 0
    # a short workspace is refused before anything is launched: y keeps its fill (as after every refusal above)
    assert mv(wb=need - 1) == -3 and mv(w=None, wb=0) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((y20 == -7.0).all()) and bool((y90 == -7.0).all())


def test_error_codes_and_refusals_of_the_kind():
    """LO_OP_KERNEL_LMC_DIAG through lo_matvec_f32 and lo_pivoted_cholesky_f32: what the descriptor may hold; the float64
    entry points refuse the kind, a sum does not take it as a term and a mask not as its base."""
    lib, p = _hip.load(), _hip.ptr
    B, n, D, Q, T, c = 1, 150, 3, 2, 2, 2
    N = n * T
    x = torch.rand(B, n, D, device=DEV)
    theta = torch.ones(B, Q, D + 1, device=DEV)
    Bt = (torch.eye(T, device=DEV) + 0.2).expand(B, Q, T, T).contiguous()
    v, y = torch.randn(B, N, c, device=DEV), torch.full((B, N, c), -7.0, device=DEV)
    st = _hip.stream_ptr(v.device)
    desc = K.kernel_lmc_diag_descriptor(x, theta, [3, 1], Bt)
    assert desc.kind == LMC and desc.n2 == 0x20013 and desc.R == D and desc.N == N
    s = desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    run = lambda: lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need, st)  # noqa: E731
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(y, K.kernel_lmc_mv(x, theta, Bt, [3, 1], v))
    y.fill_(-7.0)
    null = ctypes.cast(None, ctypes.POINTER(_hip.OpDesc))
    UNS = _hip.LO_ERR_UNSUPPORTED
    bad_desc = (("n2", 0x20043, -1), ("n2", 0x20014, -1), ("n2", -1, -1), ("n2", 0x120013, -1), ("n2", 0x00013, -1),
                ("n2", 0x10013, -1), ("n2", 0x50013, UNS), ("nterms", 0, -1), ("nterms", 7, -1), ("N", N + 1, -1),
                ("A0", None, -1), ("A1", None, -1), ("terms", null, -1), ("R", 0, -1), ("R", 33, UNS))
    for field, val, rc in bad_desc:  # (0x00013: Q = 0; 0x10013: a code beyond the Q = 1 terms; nterms 7: N % T != 0)
        s = desc.c_struct()
        setattr(s, field, val)
        assert run() == rc, (field, hex(val) if isinstance(val, int) else val)
    s = desc.c_struct()
    s.nterms, s.N = 10, 300  # (N % T == 0, T beyond LO_KERNEL_KRON_MAX_TASKS)
    assert run() == UNS
    s = desc.c_struct()
    assert lib.lo_matvec_f32(ctypes.byref(s), p(v), p(y), c, p(ws), need - 1, st) == -3
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    assert K.kernel_lmc_diag_descriptor(torch.rand(1, 10, 33, device=DEV), torch.ones(1, Q, 34, device=DEV), [0, 0], Bt) is None
    assert K.kernel_lmc_diag_descriptor(x, theta, [0, 0], torch.eye(9, device=DEV).expand(1, Q, 9, 9)) is None
    assert K.kernel_lmc_diag_descriptor(x, torch.ones(B, 5, D + 1, device=DEV), [0] * 5,
                                        torch.eye(T, device=DEV).expand(1, 5, T, T)) is None
    # the pivoted Cholesky
    L, perm = torch.empty(B, 5, N, device=DEV), torch.empty(B, N, dtype=torch.int64, device=DEV)
    rank = ctypes.c_int32(0)
    root = K.lowrank_diag_descriptor(torch.rand(B, N, 4, device=DEV), None)
    both = K.sum_descriptor([desc, root]).c_struct()
    pneed = max(lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(s), 5),
                lib.lo_pivoted_cholesky_workspace_bytes(ctypes.byref(both), 5))
    pws = torch.empty(pneed, dtype=torch.uint8, device=DEV)
    args = (5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed, st)
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == 0 and rank.value == 5
    L.fill_(-7.0)
    for field, val, rc in bad_desc:
        if field == "N":
            continue  # (the engine's own buffers are sized by N)
        s = desc.c_struct()
        setattr(s, field, val)
        assert lib.lo_pivoted_cholesky_f32(ctypes.byref(s), *args) == rc, (field, val)
    s = desc.c_struct()
    assert lib.lo_pivoted_cholesky_f64(ctypes.byref(s), 5, 1e-3, p(L), p(perm), ctypes.byref(rank), p(pws), pneed,
                                       st) == UNS
    y64 = torch.empty(B, N, c, dtype=torch.float64, device=DEV)
    assert lib.lo_matvec_f64(ctypes.byref(s), p(v.double()), p(y64), c, p(ws), need, st) < 0
    # not a term of LO_OP_SUM, not a base of LO_OP_MASKED
    sneed = lib.lo_matvec_workspace_bytes(ctypes.byref(both), c) + need
    sws = torch.empty(sneed, dtype=torch.uint8, device=DEV)
    assert lib.lo_matvec_f32(ctypes.byref(both), p(v), p(y), c, p(sws), sneed, st) == -1
    assert lib.lo_pivoted_cholesky_f32(ctypes.byref(both), *args) == -1
    idx = torch.arange(0, N, 2, device=DEV)
    assert K.masked_descriptor(desc, idx) is None
    masked = K.OperatorDescriptor(_hip.LO_OP_MASKED, B, idx.numel(), mask=(desc, idx)).c_struct()
    vm, ym = torch.randn(B, idx.numel(), c, device=DEV), torch.full((B, idx.numel(), c), -7.0, device=DEV)
    assert lib.lo_matvec_f32(ctypes.byref(masked), p(vm), p(ym), c, p(sws), sneed, st) == UNS
    torch.cuda.synchronize()
    assert bool((y == -7.0).all()) and bool((ym == -7.0).all()) and bool((L == -7.0).all())


# ---------------------------------------------------------------------------------- the goldens
def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g46_kernel_lmc_{p}.npz"))


def tensors(p, grad=False, dtype=torch.float32):
    t = {k: dev(v, dtype) for k, v in inputs(p).items()}
    if grad:
        for k in grad_names(p):
            t[k].requires_grad_(True)
    return t


def terms_of(p, t, guard=True):
    n = CASES[p][2]
    ops = []
    for q, (family, _, _) in enumerate(CASES[p][0]):
        fn = covariance.FAMILIES[family]
        kern = KernelLinearOperator(t["x"], t["x"], guarded(fn, n) if guard else fn, num_nonbatch_dimensions=NB,
                                    lengthscale=t[f"lengthscale{q}"], outputscale=t[f"outputscale{q}"])
        ops.append(KroneckerProductLinearOperator(kern, DenseLinearOperator(t[f"task{q}"])))
    return ops


def lmc_op(p, t, guard=True):
    return SumLinearOperator(*terms_of(p, t, guard))


def check(G, p, q, value):
    err, ref_err = rel(host(value), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    print(f"kernel_lmc {p} {q}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, q, err, ref_err)


def probed(p, t):
    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = t["Z"].norm(dim=-2, keepdim=True)
            return t["Z"] / n, n

    return Probed(lmc_op(p, t), DiagLinearOperator(t["noise"]))


@pytest.mark.parametrize("p", list(CASES))
def test_public_api_against_the_goldens(p):
    """(sum_q Kron(Kernel_q, B_q) + Diag) under the reference run's solver settings, covar_func guarded against any dense
    evaluation: the descriptor kind (solve and inv_quad_logdet lower to it, not to LO_OP_CALLBACK: no closure reaches
    the solvers), the product, the diagonal, solve, inv_quad_logdet with injected probes, the pivoted Cholesky, backward."""
    G = golden(p)
    terms, B, n, D, T, seed = CASES[p]
    Q = len(terms)
    with solver_settings(settings), settings.num_trace_samples(PROBES):
        t = tensors(p)
        S = lmc_op(p, t)
        A = AddedDiagLinearOperator(S, DiagLinearOperator(t["noise"]))
        desc = A._kernel_descriptor()
        assert desc is not None and desc.kind == LMC and desc.kernel_terms == T and desc.diag_mode == 1
        assert K.kernel_lmc_terms(desc) == Q and desc.A1.shape == (B, Q, D + 1) and desc.N == n * T
        assert desc.A0.data_ptr() == t["x"].data_ptr() and desc.task.shape == (B, Q, T, T)
        assert desc.n2 & 0xffff == K.kernel_sum_pack_families([covariance.FAMILIES[f].native_family for f, _, _ in terms])
        for q in range(Q):
            assert torch.equal(desc.task[:, q], t[f"task{q}"])
        assert S._kernel_descriptor().kind == LMC and S._kernel_descriptor().diag_mode == 0
        const = AddedDiagLinearOperator(S, ConstantDiagLinearOperator(t["noise"][:, :1], n * T))._kernel_descriptor()
        assert const.kind == LMC and const.diag_mode == 2
        if Q == 2:  # k1 + k2 builds a SumKroneckerLinearOperator: inside AddedDiag it takes the kind as well
            k1, k2 = terms_of(p, t)
            SK = k1 + k2
            assert isinstance(SK, SumKroneckerLinearOperator)
            dk = AddedDiagLinearOperator(SK, DiagLinearOperator(t["noise"]))._kernel_descriptor()
            assert dk is not None and dk.kind == LMC and dk.diag_mode == 1 and K.kernel_lmc_terms(dk) == 2
        check(G, p, "mv", S @ t["V"])
        check(G, p, "mv", K.kernel_lmc_mv(desc.A0, desc.A1, desc.task, [covariance.FAMILIES[f].native_family for f, _, _ in terms],
                                          t["V"]))
        check(G, p, "mv", K.matvec(S._kernel_descriptor(), t["V"]))
        check(G, p, "diag", S.diagonal())
        # the solvers get the descriptor: a product through Python (the callback route of the parent) would run the
        # terms' own products, fused (K.kernel_kron_mv) or composed (whose kernel factor calls K.kernel_mv)
        from linear_operator_amd.operators import kronecker_product_linear_operator as kp

        with mock.patch.object(kp, "_kron_matmul", side_effect=AssertionError("Python product")), \
                mock.patch.object(K, "kernel_mv", side_effect=AssertionError("Python product")), \
                mock.patch.object(K, "kernel_kron_mv", side_effect=AssertionError("Python product")), \
                mock.patch.object(K, "pivoted_cholesky_generic", side_effect=AssertionError("row fetch")):
            check(G, p, "solve", A.solve(t["rhs"]))
            if Q == 2:
                check(G, p, "solve", AddedDiagLinearOperator(SK, DiagLinearOperator(t["noise"])).solve(t["rhs"]))
            iq, ld = probed(p, t).inv_quad_logdet(t["rhs"], logdet=True)
            L, piv = S.pivoted_cholesky(RANK, return_pivots=True)
            L2, piv2 = S.pivoted_cholesky(RANK, return_pivots=True)
        check(G, p, "iq", iq)
        check(G, p, "ld", ld)
        check(G, p, "iq", A.inv_quad(t["rhs"]))
        assert np.array_equal(piv[..., :RANK].cpu().numpy(), G["piv"])
        check(G, p, "L", L)
        assert torch.equal(L, L2) and torch.equal(piv, piv2)
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(lmc_op(p, tg), DiagLinearOperator(tg["noise"]))
        Ag.inv_quad(tg["rhs"]).sum().backward()
    for name, key in grad_keys(p).items():
        check(G, p, key, tg[name].grad)


@pytest.mark.parametrize("p", list(CASES))
def test_gradients_through_inv_quad_against_fp64_autograd(p):
    """The points and every term's lengthscale, outputscale and B_q through inv_quad of the lowered operator (backward
    included) and through inv_quad_logdet, against float64 autograd on the dense matrix; the bound from the float32 run
    of the same computation (inv_quad under the same settings, autograd through the covariance functions) on the STORED
    dense operator."""
    names = grad_names(p)
    t64 = tensors(p, grad=True, dtype=torch.float64)
    A64 = dense_lmc(p, t64, covariance.FAMILIES) + torch.diag_embed(t64["noise"])
    (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum().backward()
    with solver_settings(settings):
        ts = tensors(p, grad=True)
        stored = dense_lmc(p, ts, covariance.FAMILIES)
        AddedDiagLinearOperator(DenseLinearOperator(stored), DiagLinearOperator(ts["noise"])).inv_quad(ts["rhs"]).sum().backward()
        tg = tensors(p, grad=True)
        Ag = AddedDiagLinearOperator(lmc_op(p, tg), DiagLinearOperator(tg["noise"]))
        assert Ag._kernel_descriptor().kind == LMC
        Ag.inv_quad(tg["rhs"]).sum().backward()
        tq = tensors(p, grad=True)
        iq, _ = AddedDiagLinearOperator(lmc_op(p, tq), DiagLinearOperator(tq["noise"])).inv_quad_logdet(tq["rhs"], logdet=False)
        iq.sum().backward()
    for k in names:
        want = host(t64[k].grad)
        within(f"inv_quad gradient {p} {k}", rel(host(tg[k].grad), want), rel(host(ts[k].grad), want))
        within(f"inv_quad_logdet gradient {p} {k}", rel(host(tq[k].grad), want), rel(host(ts[k].grad), want))


def test_matmul_routing_follows_the_table():
    """`_matmul` of the sum goes to the kind (lo_matvec_f32 on LO_OP_KERNEL_LMC_DIAG) exactly for the (Q, T, columns) cells
    of K._NATIVE_MATMUL_KERNEL_LMC -- as it stands, and with every cell patched on and off; every other cell keeps the
    per-term composition.  Both agree with the float64 composition either way."""
    names = ("rbf", "matern32", "matern52", "matern12")
    for Q, T in ((2, 2), (4, 4)):
        for c in (1, 5):
            B, n, D = 1, 130, 3
            fns = [covariance.FAMILIES[f] for f in names[:Q]]
            x, ls, os_, Bt, v, d = make_inputs(9900 + Q, Q, B, n, D, T, c)
            tx = dev(x)
            S = SumLinearOperator(*[
                KroneckerProductLinearOperator(
                    KernelLinearOperator(tx, tx, guarded(fns[q], n), num_nonbatch_dimensions=NB, lengthscale=dev(ls[q]),
                                         outputscale=dev(os_[q])), DenseLinearOperator(dev(Bt[:, q]))) for q in range(Q)])
            want = host(composition(fns, x, ls, os_, Bt, v, d, "none", torch.float64))
            comp = host(composition(fns, x, ls, os_, Bt, v, d, "none", torch.float32))
            cell = (Q, T, 1 if c == 1 else 2)
            for table in (dict(K._NATIVE_MATMUL_KERNEL_LMC), {cell: True}, {cell: False}, {}):
                with mock.patch.object(K, "_NATIVE_MATMUL_KERNEL_LMC", table), \
                        mock.patch.object(K, "matvec", wraps=K.matvec) as kind, \
                        mock.patch.object(K, "kernel_kron_mv", wraps=K.kernel_kron_mv) as fused, \
                        mock.patch.object(K, "kernel_mv", wraps=K.kernel_mv) as single:
                    y = S._matmul(dev(v))
                    assert S._kernel_descriptor().kind == LMC  # (the descriptor lowers whatever the table says)
                routed = bool(table.get(cell, False))
                per_term = fused.call_count + single.call_count
                assert (kind.call_count, per_term) == ((1, 0) if routed else (0, Q)), (cell, table)
                within(f"_matmul Q={Q} T={T} c={c} {'kind' if routed else 'composed'}", rel(host(y), want), rel(comp, want))


def test_product_never_holds_the_matrix():
    """n = 8192, T = 2, Q = 2, one column: the stored operator would be 1 GiB.  The allocator's peak grows by at most the
    sizer's bytes plus three copies of y, through the entry point and through the kind."""
    n, D, T, Q, c = 8192, 4, 2, 2, 1
    g = torch.Generator().manual_seed(9950)
    x = torch.rand(1, n, D, generator=g).to(DEV)
    ls = [torch.full((1, 1, D), 0.3, device=DEV), torch.full((1, 1, 1), 0.7, device=DEV)]
    os_ = [torch.full((1,), 1.2, device=DEV), torch.full((1,), 0.8, device=DEV)]
    Bt = (torch.eye(T) + 0.2 * torch.rand(Q, T, T, generator=g)).to(DEV)[None]
    v = torch.randn(1, n * T, c, generator=g).to(DEV)
    noise = (0.1 + torch.rand(1, n * T, generator=g)).to(DEV)
    theta = K.kernel_sum_theta(ls, os_, (1,), D)
    fams = [0, 3]
    allowed = _hip.load().lo_kernel_lmc_mv_workspace_bytes(1, n, D, Q, T, c) + 3 * v.numel() * 4
    assert allowed < (n * T) ** 2 * 4 // 100  # (nothing of the size of the matrix, 1 GiB)
    fns = [covariance.rbf, covariance.matern52]
    A = AddedDiagLinearOperator(SumLinearOperator(*[
        KroneckerProductLinearOperator(
            KernelLinearOperator(x, x, guarded(fns[q], n), num_nonbatch_dimensions=NB, lengthscale=ls[q], outputscale=os_[q]),
            DenseLinearOperator(Bt[:, q])) for q in range(Q)]), DiagLinearOperator(noise))
    desc = A._kernel_descriptor()
    assert desc.kind == LMC
    outs = []
    for label, call in (("entry", lambda: K.kernel_lmc_mv(x, theta, Bt, fams, v, noise)), ("kind", lambda: K.matvec(desc, v))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs.append(call())
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
        print(f"kernel_lmc_mv n={n} T={T} Q={Q} {label}: peak growth {growth} bytes, allowed {allowed}")
        assert growth <= allowed, (label, growth, allowed)
    assert torch.equal(outs[0], outs[1])
    want = 0.0
    for q in range(Q):
        rows = fns[q](x[0, :2].double(), x[0].double(), ls[q][0].double(), os_[q][0].double())  # [2, n]
        w = torch.einsum("ts,jsc->jtc", Bt[0, q].double(), v[0].double().reshape(n, T, c))
        want = want + torch.einsum("ij,jtc->itc", rows, w).reshape(2 * T, c)
    want = want + noise[0, : 2 * T, None].double() * v[0, : 2 * T].double()
    assert rel(host(outs[0][0, : 2 * T]), host(want)) <= 1e-5


def test_unchanged_behaviour_of_the_neighbouring_lowerings():
    """A sum of two Kron(Kernel, Dense) over DIFFERENT point tensors still has no descriptor and still solves correctly on
    the closure route; a single Kron(Kernel, Dense) still lowers to LO_OP_KERNEL_KRON_DIAG."""
    B, n, D, T = 1, 130, 3, 2
    x, ls, os_, Bt, v, d = make_inputs(9960, 2, B, n, D, T, 1)
    x2 = make_inputs(9961, 2, B, n, D, T, 1)[0]
    Bs = 0.5 * (Bt + Bt.transpose(0, 1, 3, 2))
    fns = [covariance.rbf, covariance.matern52]
    pts = [dev(x), dev(x2)]
    ks = [KroneckerProductLinearOperator(
        KernelLinearOperator(pts[q], pts[q], fns[q], num_nonbatch_dimensions=NB, lengthscale=dev(ls[q]), outputscale=dev(os_[q])),
        DenseLinearOperator(dev(Bs[:, q]))) for q in range(2)]
    S = SumLinearOperator(*ks)
    A = AddedDiagLinearOperator(S, DiagLinearOperator(dev(d)))
    assert S._kernel_descriptor() is None and A._kernel_descriptor() is None
    assert ks[0]._kernel_descriptor().kind == _hip.LO_OP_KERNEL_KRON_DIAG
    assert AddedDiagLinearOperator(ks[1], DiagLinearOperator(dev(d)))._kernel_descriptor().kind == _hip.LO_OP_KERNEL_KRON_DIAG
    dense = lambda dt: sum(  # noqa: E731
        dense_kron(fns[q](dev([x, x2][q], dt), dev([x, x2][q], dt), dev(ls[q], dt), dev(os_[q], dt)), dev(Bs[:, q], dt))
        for q in range(2)) + torch.diag_embed(dev(d, dt))
    want = host(torch.linalg.solve(dense(torch.float64), dev(v, torch.float64)))
    with solver_settings(settings):  # the bound: the same solve, same settings, on the STORED float32 operator
        stored = AddedDiagLinearOperator(DenseLinearOperator(dense(torch.float32) - torch.diag_embed(dev(d))),
                                         DiagLinearOperator(dev(d))).solve(dev(v))
        sol = A.solve(dev(v))
    within("closure-route solve over two point tensors", rel(host(sol), want), rel(host(stored), want))
