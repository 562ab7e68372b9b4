"""The matvec plan layer on the device, over the descriptor table of tests/matvec_plan_cases.py: a workspace of exactly
the reported size serves lo_matvec_f32 (and the CG, MINRES and Lanczos entry points), one byte less is refused before
anything is launched, and two calls give the same bits.  Tolerances are those of the kinds' own tests: low-rank 2e-6
(test_gpu_parity), dense and Kronecker 5e-6 (test_gpu_parity), sum 1e-5 (test_gpu_api), Toeplitz / SKI 2e-5
(test_gpu_ski), SKI on a grid rtol 1e-4 / atol 1e-5 (test_gpu_ski_grid), Hadamard 2e-6 of the largest entry
(test_gpu_mul), masked 1e-4 of the largest entry (test_gpu_masked)."""
import ctypes

import numpy as np
import pytest
import torch

import matvec_plan_cases as mc
from conftest import max_rel_err_cols
from linear_operator_amd import _hip as H
from linear_operator_amd import kernels as K
from oracle import lo_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LO_ERR_WORKSPACE = -3


def host(t):
    return t.detach().cpu().numpy()


def max_err(y, ref):
    return np.abs(y - ref).max() / np.abs(ref).max()


def check_product(name, y, ref):
    if name.startswith("lowrank"):
        assert max_rel_err_cols(y, ref) < 2e-6
    elif name.startswith(("dense", "kron")):
        assert max_rel_err_cols(y, ref) < 5e-6
    elif name == "sum3":
        assert max_rel_err_cols(y, ref) < 1e-5
    elif name in ("toeplitz_33", "ski", "ski_plan"):
        assert max_rel_err_cols(y, ref) <= 2e-5
    elif name.startswith("ski_grid"):
        assert np.allclose(y, ref, rtol=1e-4, atol=1e-5)
    elif name == "hadamard":
        assert max_err(y, ref) < 2e-6
    else:
        assert name.startswith("masked") and max_err(y, ref) < 1e-4


_built = {}


def built(name):
    """(case, {c: (v, float64 reference)}): built once per process and left unchanged."""
    if name not in _built:
        case = mc.build(name, DEV)
        refs = {}
        for c in mc.COLS:
            v = torch.randn(case.desc.B, case.desc.N, c, generator=torch.Generator().manual_seed(7 + c)).to(DEV)
            refs[c] = (v, host(case.product(v)))
        _built[name] = (case, refs)
    return _built[name]


def run(lib, s, v, y, c, ws, nbytes):
    rc = lib.lo_matvec_f32(ctypes.byref(s), H.ptr(v), H.ptr(y), c, H.ptr(ws), nbytes, H.stream_ptr(v.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c", mc.COLS)
@pytest.mark.parametrize("name", mc.CASES)
def test_exact_workspace_one_byte_short_and_determinism(name, c):
    lib = H.load()
    case, refs = built(name)
    v, ref = refs[c]
    s = case.desc.c_struct()
    need = lib.lo_matvec_workspace_bytes(ctypes.byref(s), c)
    assert need >= 256 + case.need(c)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    y = torch.full_like(v, 7.0)
    torch.cuda.synchronize()
    assert run(lib, s, v, y, c, ws, need - 1) == LO_ERR_WORKSPACE
    assert bool((y == 7.0).all()) and bool((ws == 0x5A).all()), "a short workspace: nothing may be launched"
    assert run(lib, s, v, y, c, ws, need) == 0
    check_product(name, host(y), ref)
    y2 = torch.full_like(v, 7.0)
    assert run(lib, s, v, y2, c, ws, need) == 0
    assert torch.equal(y, y2), "two calls differ"


@pytest.mark.parametrize("name", mc.SOLVER_CASES)
def test_solvers_on_exactly_their_reported_workspace(name):
    """K.cg_solve, K.minres_solve and K.lanczos_tridiag allocate exactly lo_cg_workspace_bytes /
    lo_minres_workspace_bytes / lo_lanczos_workspace_bytes (kernels.py); the references are the oracle's float64 runs of
    the same recurrences on the dense operator."""
    case, _ = built(name)
    A = host(case.dense)
    mv = lambda x: A @ x  # noqa: E731
    B, N = case.desc.B, case.desc.N
    rhs = torch.randn(B, N, 1, generator=torch.Generator().manual_seed(11))
    rhs64 = rhs.double().numpy()
    res = K.cg_solve(case.desc, rhs.to(DEV), max_iter=mc.CG_MAX_ITER, tolerance=1e-4)
    # (the oracle, like the reference, refuses max_tridiag_iter > max_iter even without a tridiagonal)
    xo, _, info = orc.linear_cg(mv, rhs64, max_iter=mc.CG_MAX_ITER, max_tridiag_iter=mc.CG_MAX_ITER, tolerance=1e-4)
    assert res.iterations == info.iterations
    assert max_rel_err_cols(host(res.x), xo) < 1e-4  # (test_gpu_api: a solve against the oracle's)
    shifts = torch.tensor([0.5, 2.0])
    m = K.minres_solve(case.desc, rhs.to(DEV), shifts.to(DEV), max_iter=mc.MINRES_MAX_ITER)
    mo, _ = orc.minres(mv, rhs64, shifts=shifts.double().numpy(), max_iter=mc.MINRES_MAX_ITER)
    for q in range(mc.MINRES_SHIFTS):
        assert max_rel_err_cols(host(m.x[q]), np.asarray(mo)[q]) < 5e-4  # (test_gpu_api: shifted solves)
    q_mat, t_mat = K.lanczos_tridiag(case.desc, rhs.to(DEV), mc.LANCZOS_ITERS)
    qo, to = orc.lanczos_tridiag(mv, mc.LANCZOS_ITERS, rhs64)
    t, to = host(t_mat).astype(np.float64), np.asarray(to, np.float64)
    assert t.shape == to.shape
    assert np.abs(t - to).max() <= 1e-4 * np.abs(to).max()  # (test_gpu_lanczos: tridiagonals at 1e-4 of their scale)
