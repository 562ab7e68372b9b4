"""SumKroneckerLinearOperator on the device: lo_kron_eig_apply_f32 (csrc/lo_kron_eigsolve.hip) against a float64 einsum,
and the operator's closed forms at the five cases of tests/golden/g37_sum_kron.npz against the dense float64 values
recorded there -- each within 8x the error the reference's own class had for that quantity (DESIGN.md section 6k lists
the measured ratios)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_sum_kron import CASES, GRAD_CASES, dense64, inputs  # noqa: E402

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    KroneckerProductLinearOperator, SumKroneckerLinearOperator, SumLinearOperator)

pytestmark = pytest.mark.gpu

X = inputs()
G = np.load(os.path.join(HERE, "golden", "g37_sum_kron.npz"))
DEV = "cuda"
REF_FACTOR = 8.0  # allowed multiple of the reference's own recorded error


def rel(a, b):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def eig_apply_case(seed, B, n1, n2, c):
    g = torch.Generator().manual_seed(seed)
    M1 = torch.randn(B, n1, n1, generator=g)
    S2 = torch.randn(B, n2, n2, generator=g)
    z = torch.randn(B, n1 * n2, c, generator=g)
    scale = 0.5 + torch.rand(B, n1 * n2, generator=g)
    y64 = torch.einsum("bij,bjkc,bkl->bilc", M1.double(), z.double().reshape(B, n1, n2, c), S2.double())
    return M1, S2, scale, z, y64.reshape(B, n1 * n2, c)


def column_errors(y, y64):
    """Largest relative error over the (member, column) pairs, each in the 2-norm."""
    y = y.double().cpu()
    return float(((y - y64).norm(dim=-2) / y64.norm(dim=-2)).max())


# ---------------------------------------------------------------------------------- lo_kron_eig_apply_f32
@pytest.mark.parametrize("n2", [1, 3, 5, 16, 19])
@pytest.mark.parametrize("n1", [1, 7, 33, 130])
def test_kron_eig_apply_against_fp64_einsum(n1, n2):
    tol = (n1 + n2) * 2.0 ** -23 * 4  # the fp32 dot-product bound with a factor for the two-stage product
    for B in (1, 3):
        for c in (1, 4, 17):
            M1, S2, scale, z, y64 = eig_apply_case(100 * n1 + n2 + B + c, B, n1, n2, c)
            M1, S2, scale, z = (t.to(DEV) for t in (M1, S2, scale, z))
            for sc in (scale, None):
                want = y64 * scale.double().cpu().unsqueeze(-1) if sc is not None else y64
                routes = (True, None, False) if n2 <= _hip.LO_KRON_EIG_MAX_SMALL else (None,)
                for fused in routes:  # the fused kernel, what the routing table picks, the composition
                    y = K.kron_eig_apply(M1, S2, sc, z, fused=fused)
                    assert y is not None and y.shape == z.shape
                    err = column_errors(y, want)
                    assert err <= tol, (n1, n2, B, c, sc is not None, fused, err, tol)


@pytest.mark.parametrize("n1,n2,B,c", [(8, 4, 2, 1), (260, 2, 1, 3), (512, 8, 2, 1), (256, 4, 64, 1), (256, 4, 64, 3),
                                       (64, 16, 3, 17)])
def test_kron_eig_apply_fused_on_aligned_rows_and_full_tiles(n1, n2, B, c):
    """n1 % 4 == 0: the 16-byte row loads; n1 beyond one slab of 256; 64 x 256: the 32-row workgroups."""
    M1, S2, scale, z, y64 = eig_apply_case(7 + n1 + n2, B, n1, n2, c)
    want = y64 * scale.double().unsqueeze(-1)
    y = K.kron_eig_apply(M1.to(DEV), S2.to(DEV), scale.to(DEV), z.to(DEV), fused=True)
    assert y is not None and column_errors(y, want) <= (n1 + n2) * 2.0 ** -23 * 4


def test_kron_eig_apply_on_rows_that_are_not_16_byte_aligned():
    M1, S2, scale, z, y64 = eig_apply_case(11, 2, 8, 4, 2)
    buf = torch.empty(2 * 64 + 1, device=DEV)
    view = buf[1:].view(2, 8, 8)  # contiguous, 4 bytes off a 16-byte boundary
    view.copy_(M1)
    assert view.data_ptr() % 16 == 4
    y = K.kron_eig_apply(view, S2.to(DEV), None, z.to(DEV), fused=True)
    assert column_errors(y, y64) <= 12 * 2.0 ** -23 * 4


def test_kron_eig_apply_shapes_and_limits():
    M1, S2, scale, z, y64 = eig_apply_case(3, 2, 7, 3, 2)
    M1, S2, scale, z = (t.to(DEV) for t in (M1, S2, scale, z))
    # factors shared by the batch, broadcast by the wrapper
    y = K.kron_eig_apply(M1[0], S2[0], scale, z, fused=True)
    y64b = torch.einsum("ij,bjkc,kl->bilc", M1[0].double().cpu(), z.double().cpu().reshape(2, 7, 3, 2), S2[0].double().cpu())
    assert column_errors(y, y64b.reshape(2, 21, 2) * scale.double().cpu().unsqueeze(-1)) <= 10 * 2.0 ** -23 * 4
    with pytest.raises(RuntimeError):
        K.kron_eig_apply(M1, S2, scale, z[:, :20])
    with pytest.raises(_hip.HipExtensionError):
        K.kron_eig_apply(M1.cpu(), S2, scale, z)
    lib = _hip.load()
    assert lib.lo_kron_eig_apply_workspace_bytes(2, 7, 3, 2) > 0
    assert lib.lo_kron_eig_apply_workspace_bytes(2, 7, 19, 2) > 0
    assert lib.lo_kron_eig_apply_workspace_bytes(0, 7, 3, 2) == 0
    assert lib.lo_kron_eig_apply_workspace_bytes(2, 7, 3, _hip.LO_KRON_EIG_MAX_COLS + 1) == 0
    p = _hip.ptr
    st = _hip.stream_ptr(z.device)
    y = torch.empty_like(z)
    assert lib.lo_kron_eig_apply_f32(None, p(S2), None, p(z), p(y), 2, 7, 3, 2, None, 0, st) == -1
    assert lib.lo_kron_eig_apply_f32(p(M1), p(S2), None, p(z), p(y), 2, 7, 3, 0, None, 0, st) == -1
    wide = torch.zeros(1, 21, _hip.LO_KRON_EIG_MAX_COLS + 1, device=DEV)
    assert K.kron_eig_apply(M1[:1], S2[:1], None, wide, fused=True) is None  # LO_ERR_UNSUPPORTED: the caller composes


# ---------------------------------------------------------------------------------- the operator at the golden cases
def factors(p):
    return [torch.from_numpy(X[p + "_" + k]).to(DEV) for k in "ABCD"]


def sum_kron(ts):
    return KroneckerProductLinearOperator(ts[0], ts[1]) + KroneckerProductLinearOperator(ts[2], ts[3])


def check(name, value, p, q):
    """value against the fixture's dense float64 value of quantity q of case p: at most REF_FACTOR times the reference's
    own recorded error.  Prints the ratio."""
    err, ref_err = rel(value, G[f"{p}_{q}_64"]), float(G[f"{p}_{q}_err"])
    print(f"sum_kron {p} {name}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
    assert err <= REF_FACTOR * ref_err, (p, name, err, ref_err)


@pytest.mark.parametrize("p", list(CASES))
def test_operator_solve_and_inv_quad_logdet(p):
    op = sum_kron(factors(p))
    assert type(op) is SumKroneckerLinearOperator
    for c in (1, 4):
        check(f"solve{c}", op.solve(torch.from_numpy(X[f"{p}_rhs{c}"]).to(DEV)), p, f"solve{c}")
    iq, ld = op.inv_quad_logdet(torch.from_numpy(X[p + "_rhs4"]).to(DEV), logdet=True)
    check("inv_quad", iq, p, "iq")
    print(f"sum_kron {p} logdet: err {rel(ld, G[p + '_ld_64']):.3e}")
    np.testing.assert_allclose(ld.double().cpu().numpy(), G[p + "_ld_64"], rtol=1e-5)  # (the fp64 set-up)


@pytest.mark.parametrize("p", GRAD_CASES)
def test_operator_gradients_of_the_four_factors(p):
    leaves = [t.requires_grad_(True) for t in factors(p)]
    iq, ld = sum_kron(leaves).inv_quad_logdet(torch.from_numpy(X[p + "_rhs4"]).to(DEV), logdet=True)
    (iq.sum() + ld.sum()).backward()
    for name, t in zip("ABCD", leaves):
        assert t.grad is not None and t.grad.shape == t.shape
        check("grad " + name, t.grad, p, "g" + name)


@pytest.mark.parametrize("p", list(CASES))
def test_operator_lazy_roots(p):
    op = sum_kron(factors(p))
    K64 = torch.from_numpy(dense64(X, p))
    R = op.root_decomposition().root.to_dense().double().cpu()
    Ri = op.root_inv_decomposition().root.to_dense().double().cpu()
    for name, prod, want in (("root", R @ R.mT, K64), ("root_inv", Ri @ Ri.mT, torch.linalg.inv(K64))):
        err, ref_err = rel(prod, want), float(G[f"{p}_{name}_err"])
        print(f"sum_kron {p} {name}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
        assert err <= REF_FACTOR * ref_err, (p, name, err, ref_err)


def test_operator_with_unbatched_task_factors_under_a_batch():
    """B and D of member 0 shared by the three members of case c2.  The fixture has no such case: the dense float64
    values are formed here, the bound is 8x what the reference recorded for the same quantity of case c2."""
    a, b, c, d = factors("c2")
    b0, d0 = b[0].clone().requires_grad_(True), d[0].clone().requires_grad_(True)
    op = sum_kron([a, b0, c, d0])
    assert type(op) is SumKroneckerLinearOperator and op.shape == (3, 200, 200)
    x = dict(X)
    x["c2_B"], x["c2_D"] = np.repeat(X["c2_B"][:1], 3, 0), np.repeat(X["c2_D"][:1], 3, 0)
    K64 = torch.from_numpy(dense64(x, "c2"))
    rhs = torch.from_numpy(X["c2_rhs4"])
    sol64 = torch.linalg.solve(K64, rhs.double())
    err = rel(op.solve(rhs.to(DEV)), sol64)
    print(f"sum_kron broadcast solve4: err {err:.3e}")
    assert err <= REF_FACTOR * float(G["c2_solve4_err"])
    iq, ld = op.inv_quad_logdet(rhs.to(DEV), logdet=True)
    assert rel(iq, (rhs.double() * sol64).sum((-2, -1))) <= REF_FACTOR * float(G["c2_iq_err"])
    np.testing.assert_allclose(ld.detach().double().cpu().numpy(), torch.logdet(K64).numpy(), rtol=1e-5)
    (iq.sum() + ld.sum()).backward()
    assert b0.grad.shape == (5, 5) and d0.grad.shape == (5, 5)
    l64 = [torch.from_numpy(x["c2_" + k][:1] if k in "BD" else x["c2_" + k]).double().requires_grad_(True) for k in "ABCD"]
    kron = lambda u, v: (u.unsqueeze(-1).unsqueeze(-3) * v.unsqueeze(-2).unsqueeze(-4)).reshape(  # noqa: E731
        3, u.shape[-2] * v.shape[-2], u.shape[-1] * v.shape[-1])
    k = kron(l64[0], l64[1].expand(3, 5, 5)) + kron(l64[2], l64[3].expand(3, 5, 5))
    ((rhs.double() * torch.linalg.solve(k, rhs.double())).sum() + torch.logdet(k).sum()).backward()
    assert rel(b0.grad, l64[1].grad[0]) <= REF_FACTOR * float(G["c2_gB_err"])
    assert rel(d0.grad, l64[3].grad[0]) <= REF_FACTOR * float(G["c2_gD_err"])


def test_matmul_is_still_the_sum_of_the_two_products():
    ts = factors("c2")
    op = sum_kron(ts)
    v = torch.from_numpy(X["c2_rhs4"]).to(DEV)
    want = torch.from_numpy(dense64(X, "c2")) @ v.double().cpu()
    assert column_errors(torch.matmul(op, v), want) <= (40 + 5) * 2.0 ** -23 * 4
    plain = SumLinearOperator(KroneckerProductLinearOperator(ts[0], ts[1]), KroneckerProductLinearOperator(ts[2], ts[3]))
    assert type(plain) is SumLinearOperator and not getattr(plain, "_has_closed_form_solve", False)
    assert torch.equal(torch.matmul(op, v), torch.matmul(plain, v))
