"""MaskedLinearOperator on the MI355X: the LO_OP_MASKED product (csrc/lo_masked.hip) against fp64 numpy, its routing from
the operator, and solves, inv_quad gradients, log-determinants, Lanczos and MINRES on the masked descriptor."""
import ctypes
import itertools
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_masked as gm  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import operators as ops  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator,
    LowRankRootLinearOperator, MaskedLinearOperator)
from linear_operator_amd.operators import masked_linear_operator as masked_module  # noqa: E402

pytestmark = pytest.mark.gpu
H = K._hip
HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-4  # the project's fp32-against-fp64 bar (tests/test_gpu_block.py, tests/test_gpu_mul.py)
# What `_matmul` hands to the native product, as measured: (base kind, one column / more).
ROUTED = {("dense", 1): True, ("dense", 2): False, ("kron", 1): False, ("kron", 2): False, ("sum", 1): False,
          ("sum", 2): False}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a, b = (host(a) if torch.is_tensor(a) else np.asarray(a)), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def golden(case):
    return np.load(os.path.join(HERE, "golden", f"g33_masked_{case}.npz"))


# ---------------------------------------------------------------------------------------------------- 1. the product
KRON_FACTORS = {1: (1, 1), 63: (7, 9), 257: (16, 17)}  # (the Kronecker bases have N0 = 1, 63, 272)
BASE_KINDS = ("dense", "kron", "lowrank", "sum_dense_lowrank", "sum_kron_lowrank")


def base_members(kind, seed, B, N0, diag):
    """(descriptor of the base with its diagonal, the base matrices in fp64 [B, n, n])."""
    r = np.random.default_rng(seed)
    n1, n2 = KRON_FACTORS[N0]
    n = n1 * n2 if "kron" in kind else N0
    terms, A64 = [], np.zeros((B, n, n))
    if kind in ("dense", "sum_dense_lowrank"):
        A = (r.standard_normal((B, n, n)) / np.sqrt(n)).astype(np.float32)
        terms.append(K.dense_diag_descriptor(dev(A), None))
        A64 = A64 + A.astype(np.float64)
    if "kron" in kind:
        A1 = (r.standard_normal((B, n1, n1)) / np.sqrt(n1)).astype(np.float32)
        A2 = (r.standard_normal((B, n2, n2)) / np.sqrt(n2)).astype(np.float32)
        terms.append(K.kron_diag_descriptor(dev(A1), dev(A2), None))
        A64 = A64 + np.einsum("bij,bkl->bikjl", A1.astype(np.float64), A2.astype(np.float64)).reshape(B, n, n)
    if "lowrank" in kind:
        R = 5 if kind == "lowrank" else 8  # (5: the padded copy of the root)
        C = (r.standard_normal((B, n, R)) / np.sqrt(R)).astype(np.float32)
        terms.append(K.lowrank_diag_descriptor(dev(C), None))
        A64 = A64 + C.astype(np.float64) @ C.astype(np.float64).swapaxes(-1, -2)
    d = None
    if diag == "full":
        d = (0.5 + r.random((B, n))).astype(np.float32)
        A64 = A64 + np.einsum("bi,ij->bij", d.astype(np.float64), np.eye(n))
    elif diag == "const":
        d = (0.5 + r.random(B)).astype(np.float32)
        A64 = A64 + d.astype(np.float64)[:, None, None] * np.eye(n)
    desc = terms[0] if len(terms) == 1 else K.sum_descriptor(terms)
    if d is not None:
        desc = K._with_diag(desc, dev(d), diag == "const")
    return desc, A64


def masks_of(n, seed):
    r = np.random.default_rng(seed)
    out = {"all": np.ones(n, bool)}
    one = np.zeros(n, bool)
    one[n // 2] = True
    out["one"] = one
    ends = np.zeros(n, bool)
    ends[[0, n - 1]] = True
    out["ends"] = ends
    out["every_other"] = np.arange(n) % 2 == 0
    out["prefix"] = np.arange(n) < max(1, n // 3)
    rnd = r.random(n) < 0.7
    rnd[r.integers(n)] = True
    out["random70"] = rnd
    if n >= 65:
        m65 = np.zeros(n, bool)
        m65[r.permutation(n)[:65]] = True
        out["m65"] = m65
    seen, uniq = set(), {}
    for k, m in out.items():  # (at N0 = 1 all of them are the same mask)
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            uniq[k] = m
    return uniq


@pytest.mark.parametrize("kind", BASE_KINDS)
def test_native_matvec_against_fp64(kind):
    worst, count = 0.0, 0
    for i, (diag, N0, B) in enumerate(itertools.product(("none", "full", "const"), (1, 63, 257), (1, 3))):
        base, A64 = base_members(kind, 100 + i, B, N0, diag)
        n = A64.shape[-1]
        for name, mask in masks_of(n, 200 + i).items():
            idx = np.nonzero(mask)[0]
            M = idx.size
            S64 = A64[:, idx][:, :, idx]
            for outer, c in itertools.product(("none", "full"), (1, 2, 17, 33)):
                r = np.random.default_rng(1000 * i + 7 * c + M)
                v = r.standard_normal((B, M, c)).astype(np.float32)
                d = (0.5 + r.random((B, M))).astype(np.float32) if outer == "full" else None
                desc = K.masked_descriptor(base, dev(idx), None if d is None else dev(d))
                assert desc.kind == H.LO_OP_MASKED and desc.N == M and desc.B == B
                y64 = S64 @ v.astype(np.float64)
                if d is not None:
                    y64 = y64 + d.astype(np.float64)[..., None] * v
                err = relerr(K.matvec(desc, dev(v)), y64)
                worst, count = max(worst, err), count + 1
                assert err < BAR, (kind, diag, N0, B, name, outer, c, err)
    print(f"{kind}: {count} products, worst relative error {worst:.2e}")


def test_index_outside_the_base_contributes_nothing():
    base, A64 = base_members("dense", 5, 2, 63, "full")
    kron, K64 = base_members("kron", 6, 2, 63, "const")
    for b, B64 in ((base, A64), (kron, K64)):
        idx = np.array([0, 5, 17, 62, 63, 1000], np.int64)  # (strictly increasing; the last two lie outside)
        v = np.random.default_rng(1).standard_normal((2, 6, 2)).astype(np.float32)
        y = host(K.matvec(K.masked_descriptor(b, dev(idx)), dev(v)))
        y64 = B64[:, idx[:4]][:, :, idx[:4]] @ v[:, :4].astype(np.float64)
        assert relerr(y[:, :4], y64) < BAR and np.all(y[:, 4:] == 0.0)


def test_unsupported_bases_and_pivoted_cholesky():
    F = torch.randn(1, 16, 3, device="cuda")
    idx = torch.arange(0, 16, 2, device="cuda")
    assert K.masked_descriptor(K.hadamard_diag_descriptor(F, F, None), idx) is None
    inner = K.masked_descriptor(K.dense_diag_descriptor(torch.randn(1, 16, 16, device="cuda"), None), idx)
    assert K.masked_descriptor(inner, torch.arange(4, device="cuda")) is None
    # the C side refuses them too
    bad = K.OperatorDescriptor(H.LO_OP_MASKED, 1, 8, batch_shape=torch.Size([1]),
                               mask=(K.hadamard_diag_descriptor(F, F, None), idx))
    s = bad.c_struct()
    v = torch.randn(1, 8, 1, device="cuda")
    lib = H.load()
    ws = H.workspace(1 << 16, "cuda")
    rc = lib.lo_matvec_f32(ctypes.byref(s), H.ptr(v), H.ptr(torch.empty_like(v)), 1, H.ptr(ws), ws.numel(),
                           H.stream_ptr("cuda"))
    assert rc == H.LO_ERR_UNSUPPORTED
    with pytest.raises(H.HipExtensionError, match="unsupported"):
        K.pivoted_cholesky(inner, 4)


# ---------------------------------------------------------------------------------------------------- 2. routing
def route_operator(kind, n0=96):
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    if kind == "dense":
        base = DenseLinearOperator(rn(2, n0, n0) / n0 ** 0.5)
    elif kind == "kron":
        base = KroneckerProductLinearOperator(DenseLinearOperator(rn(2, 12, 12) / 3), DenseLinearOperator(rn(2, 8, 8) / 3))
    else:
        base = DenseLinearOperator(rn(2, n0, n0) / n0 ** 0.5) + LowRankRootLinearOperator(rn(2, n0, 4))
    mask = torch.rand(n0, device="cuda", generator=g) < 0.7
    return MaskedLinearOperator(base, mask, mask)


@pytest.mark.parametrize("kind", ["dense", "kron", "sum"])
def test_matmul_routing(kind):
    A = route_operator(kind)
    assert A._kernel_descriptor().kind == H.LO_OP_MASKED
    dense = A.to_dense().double()
    assert {k for k, v in masked_module._NATIVE_MATMUL.items() if v} == {k for k, v in ROUTED.items() if v}
    for c in (1, 17):
        v = torch.randn(2, A.size(-1), c, device="cuda")
        with mock.patch.object(K, "matvec", wraps=K.matvec) as mv:
            y = A._matmul(v)
            native = any(call.args[0].kind == H.LO_OP_MASKED for call in mv.call_args_list)
        assert native == ROUTED[(kind, 1 if c == 1 else 2)], (kind, c)
        yc = A._matmul_composition(v)
        assert relerr(y, host(dense @ v.double())) < BAR and relerr(yc, host(dense @ v.double())) < BAR


def test_lowrank_base_lowers_to_a_gathered_root():
    g = torch.Generator(device="cuda").manual_seed(4)
    C = torch.randn(2, 300, 8, device="cuda", generator=g)
    d = torch.rand(2, 300, device="cuda", generator=g) + 0.5
    mask = torch.rand(300, device="cuda", generator=g) < 0.7
    A = MaskedLinearOperator(LowRankRootLinearOperator(C) + DiagLinearOperator(d), mask, mask)
    desc = A._kernel_descriptor()
    M = int(mask.sum())
    assert desc.kind == H.LO_OP_LOWRANK_DIAG and desc.N == M and desc.diag_mode == H.LO_DIAG_FULL and not desc.mask
    assert A._kernel_descriptor().A0 is desc.A0  # the gathered copy is kept
    full = (C.double() @ C.double().mT + torch.diag_embed(d.double()))[:, mask][:, :, mask]
    v = torch.randn(2, M, 3, device="cuda", generator=g)
    assert relerr(A._matmul(v), host(full @ v.double())) < BAR
    assert relerr(A.solve(v), host(torch.linalg.solve(full, v.double()))) < BAR


def test_no_descriptor_for_nonsquare_fp64_cpu():
    A = route_operator("dense")
    other = A.row_mask.clone()
    other[:3] = ~other[:3]
    assert MaskedLinearOperator(A.base, A.row_mask, other)._kernel_descriptor() is None
    assert A.to(torch.float64)._kernel_descriptor() is None
    assert A.to("cpu")._kernel_descriptor() is None
    R = MaskedLinearOperator(A.base, A.row_mask, other)
    v = torch.randn(2, R.size(-1), 2, device="cuda")
    assert relerr(R._matmul(v), host(R.to_dense().double() @ v.double())) < BAR


# ---------------------------------------------------------------------------------------------------- 3. solves
def golden_operator(case, requires_grad=False):
    x = gm.masked_inputs(case)
    t = {k: dev(x[k]).requires_grad_(requires_grad) for k in gm.GRAD_NAMES[case]}
    mask = dev(x["mask"])
    return x, t, MaskedLinearOperator(gm.build_base(ops, case, t), mask, mask)


def cg_settings(g):
    return (settings.max_cholesky_size(0), settings.cg_tolerance(float(g["cg_tol"])), settings.max_cg_iterations(200))


@pytest.mark.parametrize("case", ["kron", "dense"])
def test_solve_on_the_streaming_engine(case):
    g = golden(case)
    x, t, A = golden_operator(case)
    assert A._kernel_descriptor().kind == H.LO_OP_MASKED
    bar = max(BAR, 2 * float(g["solve_referr"]))
    a, b, c = cg_settings(g)
    with a, b, c, mock.patch.object(K, "cg_solve", wraps=K.cg_solve) as cg:
        sol = A.solve(dev(x["rhs"]))
        plan = K.cg_last_executed()
    err = relerr(sol, g["solve_exact"])
    print(f"{case}: solve error {err:.2e} (bar {bar:.2e}, reference {float(g['solve_referr']):.2e})")
    assert err < bar
    assert cg.call_count == 1 and cg.call_args.args[0].kind == H.LO_OP_MASKED
    assert not plan["resident"] and plan["serial_engine"] == "none" and plan["rspace"] == "none" \
        and plan["lockstep_cols"] == 0, plan


def test_solve_iterations_below_the_cap():
    g = golden("kron")
    x, t, A = golden_operator("kron")
    res = K.cg_solve(A._kernel_descriptor(), dev(x["rhs"]), max_iter=200, tolerance=float(g["cg_tol"]))
    assert 0 < res.iterations < 200 and res.tolerance_reached
    assert relerr(res.x, g["solve_exact"]) < max(BAR, 2 * float(g["solve_referr"]))


def test_added_diag_solve_with_the_generic_pivoted_cholesky():
    x = gm.masked_inputs("dense")
    mask = dev(x["mask"])
    A = MaskedLinearOperator(DenseLinearOperator(dev(x["K"])), mask, mask)
    d = dev(x["D"])[:, : A.size(-1)].contiguous()
    S = AddedDiagLinearOperator(A, DiagLinearOperator(d))
    desc = S._kernel_descriptor()
    assert desc.kind == H.LO_OP_MASKED and desc.diag_mode == H.LO_DIAG_FULL
    full = A.to_dense().double() + torch.diag_embed(d.double())
    rhs = dev(x["rhs"])
    with settings.max_cholesky_size(0), settings.min_preconditioning_size(8), settings.max_preconditioner_size(5), \
            settings.cg_tolerance(1e-5), mock.patch.object(K, "pivoted_cholesky_generic",
                                                           wraps=K.pivoted_cholesky_generic) as pc:
        sol = S.solve(rhs)
    assert pc.call_count == 1
    assert relerr(sol, host(torch.linalg.solve(full, rhs.double()))) < BAR


# ---------------------------------------------------------------------------------------------------- 4. gradients
@pytest.mark.parametrize("case", gm.CASES)
def test_inv_quad_and_gradients(case):
    g = golden(case)
    x, t, A = golden_operator(case, requires_grad=True)
    a, b, c = cg_settings(g)
    with a, b, c:
        iq = A.inv_quad(dev(x["rhs"]))
        iq.sum().backward()
    bar = max(BAR, 2 * float(g["inv_quad_referr"]))
    err = relerr(iq, g["inv_quad_exact"])
    print(f"{case}: inv_quad error {err:.2e} (bar {bar:.2e})")
    assert err < bar
    for k in gm.GRAD_NAMES[case]:
        bar = max(BAR, 2 * float(g[f"grad_{k}_referr"]))
        err = relerr(t[k].grad, g[f"grad_{k}_exact"].astype(np.float64))
        print(f"{case}: gradient {k} error {err:.2e} (bar {bar:.2e})")
        assert err < bar


# ---------------------------------------------------------------------------------------------------- 5. logdet
@pytest.mark.parametrize("case", ["kron", "dense"])
def test_inv_quad_logdet_native_against_composition(case):
    g = golden(case)
    x, t, A = golden_operator(case)
    rhs = dev(x["rhs"])

    def run():
        torch.manual_seed(11)
        with settings.max_cholesky_size(0), settings.cg_tolerance(float(g["cg_tol"])), settings.num_trace_samples(16):
            return A.inv_quad_logdet(rhs, logdet=True)

    iq, ld = run()
    with mock.patch.object(MaskedLinearOperator, "_kernel_descriptor", return_value=None), \
            mock.patch.object(MaskedLinearOperator, "_matmul", MaskedLinearOperator._matmul_composition):
        iq_c, ld_c = run()
    assert relerr(iq, host(iq_c)) < BAR and relerr(ld, host(ld_c)) < BAR, (host(ld), host(ld_c))


# ---------------------------------------------------------------------------------------------------- 6. Lanczos, MINRES
def test_lanczos_and_minres_against_the_closure():
    x, t, A = golden_operator("kron")
    desc = A._kernel_descriptor()
    closure = lambda v: A._matmul_composition(v)  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(9)
    init = torch.randn(2, A.size(-1), 3, device="cuda", generator=g)
    q, tm = K.lanczos_tridiag(desc, init, 12)
    qc, tc = K.lanczos_tridiag(None, init, 12, matvec_closure=closure)
    assert tm.shape == tc.shape and relerr(tm, host(tc)) < BAR
    rhs = dev(x["rhs"])
    shifts = torch.tensor([0.0, 0.5], device="cuda")
    res = K.minres_solve(desc, rhs, shifts, max_iter=60, tolerance=1e-6)
    ref = K.minres_solve(None, rhs, shifts, matvec_closure=closure, max_iter=60, tolerance=1e-6)
    assert relerr(res.x, host(ref.x)) < BAR
    full = A.to_dense().double()
    assert relerr(res.x[0], host(torch.linalg.solve(full, rhs.double()))) < BAR


# ---------------------------------------------------------------------------------------------------- 7. workspace
@pytest.mark.parametrize("kind", ["dense", "kron"])
def test_short_workspace_is_refused_before_any_launch(kind):
    base, _ = base_members(kind, 1, 2, 63, "none")
    n = base.N
    desc = K.masked_descriptor(base, torch.arange(0, n, 2, device="cuda"))
    s = desc.c_struct()
    lib = H.load()
    c = 2
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    assert need > 4 * 2 * n * c
    v = torch.randn(2, desc.N, c, device="cuda")
    y = torch.full_like(v, 7.0)
    ws = H.workspace(need, "cuda")
    ws.fill_(0x5A)
    torch.cuda.synchronize()
    rc = lib.lo_matvec_f32(ctypes.byref(s), H.ptr(v), H.ptr(y), c, H.ptr(ws), need - 1, H.stream_ptr("cuda"))
    torch.cuda.synchronize()
    assert rc == -3  # LO_ERR_WORKSPACE
    assert bool((y == 7.0).all()) and bool((ws == 0x5A).all()), "nothing was launched"
    rc = lib.lo_matvec_f32(ctypes.byref(s), H.ptr(v), H.ptr(y), c, H.ptr(ws), need, H.stream_ptr("cuda"))
    assert rc == 0 and not bool((y == 7.0).any())
