"""lo_kernel_param_bilinear_wide_f32 / _points_grad_wide_f32 and lo_kernel_sm_bilinear_wide_f32 / _points_grad_wide_f32
(csrc/lo_kernel_kinds_bil_wide.hip: W = U V^T on v_mfma_f32_32x32x2_f32, the pair work once per pair and sweep of 32
columns) on the MI355X against float64 autograd through the dense function, under the bound of
tests/test_gpu_kernel_param.py and test_gpu_kernel_sm.py (their `within`: at most 4 times the error of float32 autograd
on the same inputs, floored at ERR_FLOOR); every case prints its ratios."""
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_kernel_param as P
import test_gpu_kernel_sm as S

from linear_operator_amd import _hip, covariance
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import KernelLinearOperator

pytestmark = pytest.mark.gpu

DEV, dev, host, rel = P.DEV, P.dev, P.host, P.rel

# M: the 32-row tile and the half-wave swap, a second wave, a second workgroup; N: the 32-point block, the 128-point tile,
# js > 1 (N > 128); t: an odd last contraction step, a full sweep of 32, a second and a third sweep; B = 512: no column
# split.  (family, B, M, N, D, t, ARD, span): both families meet every padded dimension
PARAM_CASES = [
    ("rq", 1, 1, 2, 1, 1, True, 3.0), ("rq", 1, 31, 3, 3, 3, False, 3.0), ("rq", 3, 33, 31, 8, 8, True, 3.0),
    ("rq", 1, 65, 33, 16, 9, True, 3.0), ("rq", 1, 257, 127, 32, 17, False, 3.0), ("rq", 1, 33, 129, 3, 32, True, 3.0),
    ("rq", 1, 65, 257, 8, 33, True, 3.0), ("rq", 1, 31, 257, 1, 65, True, 3.0), ("rq", 1, 130, 77, 3, 17, True, 3.0),
    ("rq", 512, 33, 33, 3, 9, True, 3.0),
    ("periodic", 1, 1, 3, 3, 1, True, 3.0), ("periodic", 3, 31, 2, 1, 3, True, 3.0),
    ("periodic", 1, 33, 31, 8, 8, False, 3.0), ("periodic", 1, 65, 33, 16, 17, True, 3.0),
    ("periodic", 1, 257, 127, 32, 9, True, 3.0), ("periodic", 1, 33, 129, 32, 33, False, 3.0),
    ("periodic", 1, 65, 257, 3, 65, True, 3.0), ("periodic", 1, 130, 77, 8, 32, True, 3.0),
    ("periodic", 512, 33, 33, 1, 17, True, 3.0), ("periodic", 2, 257, 257, 2, 17, True, 800.0),
]
# (B, M, N, D, Q, t, span): D 1 / 3 / 5 / 16 and Q 1 / 3 / 16; every padded dimension meets an odd t and a second sweep
SM_CASES = [
    (1, 1, 2, 1, 1, 1, 3.0), (1, 31, 3, 3, 3, 3, 3.0), (3, 33, 31, 1, 3, 33, 3.0), (1, 65, 33, 3, 1, 8, 3.0),
    (1, 257, 127, 5, 3, 9, 3.0), (1, 33, 129, 5, 1, 65, 3.0), (1, 65, 257, 16, 3, 17, 3.0), (1, 31, 257, 16, 1, 33, 3.0),
    (1, 33, 33, 16, 16, 32, 3.0), (1, 130, 77, 3, 16, 17, 3.0), (512, 33, 33, 1, 1, 9, 3.0), (1, 257, 257, 3, 3, 17, 3.0),
    (1, 65, 31, 5, 16, 3, 3.0), (2, 257, 257, 2, 2, 17, 2400.0),
]


def columns(seed, B, M, N, t):
    g = P.rng(seed)
    return g.standard_normal((B, M, t)).astype(np.float32), g.standard_normal((B, N, t)).astype(np.float32)


def ident(case):
    return "-".join(str(x) for x in case)


@pytest.mark.parametrize("case", PARAM_CASES, ids=ident)
def test_param_derivatives_against_fp64_autograd(case):
    family, B, M, N, D, t, ard, span = case
    x1, x2, ls, os_, sh, _, _ = P.make_inputs(9700 + PARAM_CASES.index(case), family, B, M, N, D, 1, ard, span)
    if span > 600:
        assert ((x1.max(1) - x1.min(1)) / sh[:, 0]).min() > 600
    U, V = columns(9750, B, M, N, t)
    x2 = x1.copy() if M == N else x2  # (as autograd leaves the two sides are apart, as the entry points hold them)
    want = P.autograd_all(family, x1, x2, ls, os_, sh, U, V, torch.float64)
    ref = P.autograd_all(family, x1, x2, ls, os_, sh, U, V, torch.float32)
    tx1, tx2, tU, tV = dev(x1), dev(x2), dev(U), dev(V)
    lead = (P.theta_of(family, ls, os_, sh, D), covariance.PARAM_FAMILIES[family].native_family)
    g_theta = K.kernel_param_bilinear_wide(tx1, tx2, *lead, tU, tV)
    g_x1 = K.kernel_param_points_grad_wide(tx1, tx2, *lead, tU, tV)
    g_x2 = K.kernel_param_points_grad_wide(tx2, tx1, *lead, tV, tU)
    assert g_theta.shape == (B, 2 * D + 2) and g_x1.shape == (B, M, D) and g_x2.shape == (B, N, D)
    unread = slice(D + 2, 2 * D + 2) if family == "rq" else slice(D + 1, D + 2)
    assert not g_theta[:, unread].any()  # (the slots the family does not read: written as 0)
    own = slice(D + 1, D + 2) if family == "rq" else slice(D + 2, 2 * D + 2)
    for what, got, w, r in (("lengthscale slots", g_theta[:, :D], want[0][:, :D], ref[0][:, :D]),
                            ("os2 slot", g_theta[:, D], want[0][:, D], ref[0][:, D]),
                            ("alpha slot" if family == "rq" else "period slots", g_theta[:, own], want[0][:, own], ref[0][:, own]),
                            ("x1", g_x1, want[1], ref[1]), ("x2", g_x2, want[2], ref[2])):
        assert torch.isfinite(got).all()
        P.within(f"wide {what} {ident(case)}", rel(host(got), w), rel(r, w))
    assert torch.equal(K.kernel_param_bilinear_wide(tx1, tx2, *lead, tU, tV), g_theta)  # two calls: equal bits
    assert torch.equal(K.kernel_param_points_grad_wide(tx1, tx2, *lead, tU, tV), g_x1)


@pytest.mark.parametrize("case", SM_CASES, ids=ident)
def test_sm_derivatives_against_fp64_autograd(case):
    B, M, N, D, Q, t, span = case
    x1, x2, w, mu, sg, _, _ = S.make_inputs(9800 + SM_CASES.index(case), B, M, N, D, Q, 1, span)
    if span > 600:  # every member's points span more than 600 periods of its fastest mixture
        assert ((x1.max(1) - x1.min(1))[:, None, :] * mu).max((1, 2)).min() > 600
    U, V = columns(9850, B, M, N, t)
    x2 = x1.copy() if M == N else x2
    want = S.autograd_all(x1, x2, w, mu, sg, U, V, torch.float64)
    ref = S.autograd_all(x1, x2, w, mu, sg, U, V, torch.float32)
    tx1, tx2, tU, tV, theta = dev(x1), dev(x2), dev(U), dev(V), S.theta_of(w, mu, sg)
    g_theta = K.kernel_sm_bilinear_wide(tx1, tx2, theta, tU, tV)
    g_x1 = K.kernel_sm_points_grad_wide(tx1, tx2, theta, tU, tV)
    g_x2 = K.kernel_sm_points_grad_wide(tx2, tx1, theta, tV, tU)
    assert g_theta.shape == (B, Q, 2 * D + 1) and g_x1.shape == (B, M, D) and g_x2.shape == (B, N, D)
    for what, got, wnt, r in (("weights", g_theta[..., 0], want[0][..., 0], ref[0][..., 0]),
                              ("means", g_theta[..., 1:1 + D], want[0][..., 1:1 + D], ref[0][..., 1:1 + D]),
                              ("scales", g_theta[..., 1 + D:], want[0][..., 1 + D:], ref[0][..., 1 + D:]),
                              ("x1", g_x1, want[1], ref[1]), ("x2", g_x2, want[2], ref[2])):
        assert torch.isfinite(got).all()
        S.within(f"wide {what} {ident(case)}", rel(host(got), wnt), rel(r, wnt))
    assert torch.equal(K.kernel_sm_bilinear_wide(tx1, tx2, theta, tU, tV), g_theta)  # two calls: equal bits
    assert torch.equal(K.kernel_sm_points_grad_wide(tx1, tx2, theta, tU, tV), g_x1)


@pytest.mark.parametrize("stem", ["lo_kernel_param_bilinear", "lo_kernel_param_points_grad", "lo_kernel_sm_bilinear",
                                  "lo_kernel_sm_points_grad"])
def test_wide_entry_points_return_the_error_codes_of_their_twins(stem):
    lib, p = _hip.load(), _hip.ptr
    B, M, D, t, sm = 1, 300, 3, 17, "_sm_" in stem
    x, U = torch.rand(B, M, D, device=DEV), torch.randn(B, M, t, device=DEV)
    theta = torch.ones(B, 2 * (2 * D + 1) if sm else 2 * D + 2, device=DEV)
    g = torch.full((B, M, 2 * D + 2), -7.0, device=DEV)  # (room for either output)
    st = _hip.stream_ptr(x.device)
    sizer = getattr(lib, stem + "_wide_workspace_bytes")
    need = sizer(B, M, M, D, 2, t) if sm else sizer(B, M, M, D, t)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def both(x1=x, second=2 if sm else _hip.LO_KERNEL_RQ, dim=D, w=ws, wb=need):  # second: Q or the family
        a = (p(x1), p(x), p(theta), second, B, M, M, dim, p(U), p(U), t, p(g), p(w), wb, st)
        codes = getattr(lib, stem + "_wide_f32")(*a), getattr(lib, stem + "_f32")(*a)
        assert codes[0] == codes[1], codes
        return codes[0]

    assert need > 256 and both(x1=None) == -1 and both(dim=17 if sm else 33) == _hip.LO_ERR_UNSUPPORTED
    assert both(second=17 if sm else 3) == (_hip.LO_ERR_UNSUPPORTED if sm else -1)  # (Q = 17; a family of the plain kind)
    assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: g keeps its fill
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and both() == 0


def routed(op, kind, t, suffix, seed):
    """Whether every gradient of op._bilinear_derivative with t columns has the bits of the entries kernel_<kind>_*<suffix>."""
    n = op.shape[-1]
    g = torch.Generator(device=DEV).manual_seed(seed)
    U, V = torch.randn(3, n, t, device=DEV, generator=g), torch.randn(3, n, t, device=DEV, generator=g)
    own = op._bilinear_derivative(U, V)
    with mock.patch.object(K, f"kernel_{kind}_bilinear", getattr(K, f"kernel_{kind}_bilinear{suffix}")), \
            mock.patch.object(K, f"kernel_{kind}_points_grad", getattr(K, f"kernel_{kind}_points_grad{suffix}")):
        direct = op._bilinear_derivative(U, V)
    return all(a is not None and torch.equal(a, b) for a, b in zip(own, direct))


@pytest.mark.parametrize("family", ["rq", "periodic", "sm"])
def test_the_operator_takes_the_wide_kernels_where_the_rule_says_so(family):
    """The route through the run functions of the plain entries (kp_bil_wide / ksm_bil_wide of csrc/lo_kernel_shape.h), the
    dense function guarded: at t = 17, a routed cell of every family at D = 3, every gradient has the bits of the wide
    entries; at t = 4 those of the plain entries, which there are not the wide entries' bits (the two kernels sum W and the
    one-number slots differently, so the comparison tells the routes apart)."""
    B, n, D = 3, 300, 3
    if family == "sm":
        x1, _, w, mu, sg, _, _ = S.make_inputs(9901, B, n, n, D, 2, 1)
        params = dict(mixture_weights=dev(w), mixture_means=dev(mu), mixture_scales=dev(sg))
        fn, nb, kind = S.guarded(n), S.NB, "sm"
    else:
        x1, _, ls, os_, sh, _, _ = P.make_inputs(9900, family, B, n, n, D, 1)
        params = {"lengthscale": dev(ls), "outputscale": dev(os_), P.SHAPE[family]: dev(sh)}
        fn, nb, kind = P.guarded(covariance.PARAM_FAMILIES[family], n), P.NB, "param"
    tx = dev(x1).requires_grad_(True)
    op = KernelLinearOperator(tx, tx, fn, num_nonbatch_dimensions=nb, **{k: v.requires_grad_(True) for k, v in params.items()})
    assert routed(op, kind, 17, "_wide", 9902)
    assert routed(op, kind, 4, "", 9903) and not routed(op, kind, 4, "_wide", 9903)
