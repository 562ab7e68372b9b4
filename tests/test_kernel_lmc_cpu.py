"""The matrix-free LMC operator sum_q Kron(Kernel_q, Dense(B_q)) without a GPU: the binding of ABI 38 (symbols, constants,
the struct of the kind, the host-side sizer against the closed form of its layout), the gate of the lowering decided on
CPU tensors through its `check_device=False` form, and the reference's goldens (tests/golden/g46_kernel_lmc_*.npz)
against the float64 dense composition of the covariance functions."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_lmc import CASES, ERR_FLOOR, RANK, dense_lmc, grad_keys, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, RootLinearOperator, SumLinearOperator)
from linear_operator_amd.operators.sum_linear_operator import _lmc_terms  # noqa: E402

REF_FACTOR = 4.0
NB = {"outputscale": 0}


def kron(x, Bt, name="rbf", ls=0.6):
    D = x.shape[-1]
    kern = KernelLinearOperator(x, x, covariance.FAMILIES[name], num_nonbatch_dimensions=NB,
                                lengthscale=torch.full((1, D), ls), outputscale=torch.tensor(1.1))
    return KroneckerProductLinearOperator(kern, DenseLinearOperator(Bt))


def split_count(B, n):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-n // 256), -(-n // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return -(-n // jchunk)


def test_binding_of_abi_38():
    assert _hip.ABI_VERSION >= 38 and _hip.LO_OP_KERNEL_LMC_DIAG == 17
    assert _hip.LO_KERNEL_MAX_TERMS == 4 and _hip.LO_KERNEL_KRON_MAX_TASKS == 8
    assert "lo_kernel_lmc_mv_workspace_bytes" in _hip.EXPORTS and "lo_kernel_lmc_mv_f32" in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["lo_kernel_lmc_mv_workspace_bytes"][1]) == 6
    assert len(_hip._PROTOTYPES["lo_kernel_lmc_mv_f32"][1]) == 17
    assert callable(K.kernel_lmc_diag_descriptor) and callable(K.kernel_lmc_mv)
    lib = _hip.load()  # (the sizer is host code)
    assert lib.lo_abi_version() == _hip.ABI_VERSION


def test_struct_of_the_kind():
    """T rides in `nterms`, the Q family codes in the low bits of n2 with Q itself in bits 16 .. 19, the union slot holds
    the device pointer of Bt [B, Q, T, T] as given; the struct has the size it had."""
    Bt = torch.eye(3).expand(2, 2, 3, 3).contiguous()
    n2 = K.kernel_sum_pack_families([3, 1]) | (2 << 16)
    assert n2 == 0x20013
    desc = K.OperatorDescriptor(_hip.LO_OP_KERNEL_LMC_DIAG, 2, 30, R=4, n2=n2, kernel_terms=3, task=Bt)
    s = desc.c_struct()
    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (17, 3, 0x20013, 4, 30)
    assert ctypes.cast(s.terms, ctypes.c_void_p).value == Bt.data_ptr()
    assert K.kernel_lmc_terms(desc) == 2
    assert desc.without_diag().task is Bt and desc.without_diag().kernel_terms == 3 and desc.without_diag().n2 == n2
    assert ctypes.sizeof(_hip.OpDesc) == 80  # (kind, diag_mode, B, N, R, n2, A0, A1, d, nterms, reserved, the union)


@pytest.mark.parametrize("B,n,D,Q,T,c", [(512, 40, 2, 2, 2, 2), (128, 1024, 1, 4, 8, 17), (1, 1, 1, 1, 1, 1),
                                         (1, 300, 8, 4, 3, 17), (3, 257, 3, 2, 2, 1), (1, 16384, 4, 2, 4, 1),
                                         (8, 4096, 16, 3, 8, 17)])
def test_sizer_is_the_closed_form_of_the_layout(B, n, D, Q, T, c):
    """The tail alone without a split; with one, js copies of the product [B, n T, c] -- whatever Q is."""
    lib = _hip.load()
    js = split_count(B, n)
    want = 256 + (4 * js * B * n * T * c if js > 1 else 0)
    assert lib.lo_kernel_lmc_mv_workspace_bytes(B, n, D, Q, T, c) == want
    assert lib.lo_kernel_lmc_mv_workspace_bytes(B, n, D, 1, T, c) == lib.lo_kernel_kron_mv_workspace_bytes(B, n, D, T, c)
    if (B, n) in ((512, 40), (128, 1024), (1, 1)):
        assert js == 1
    if (B, n) in ((1, 300), (3, 257), (1, 16384)):
        assert js > 1


def test_sizer_refuses_what_the_entry_point_refuses():
    lib = _hip.load()
    for args in ((1, 10, 33, 2, 2, 1), (1, 10, 3, 5, 2, 1), (1, 10, 3, 0, 2, 1), (1, 10, 3, 2, 9, 1), (1, 10, 3, 2, 0, 1),
                 (0, 10, 3, 2, 2, 1), (1, 0, 3, 2, 2, 1), (1, 10, 0, 2, 2, 1), (1, 10, 3, 2, 2, 0), (65536, 10, 3, 2, 2, 1),
                 (1, 0x7ffffe01, 3, 2, 1, 1), (1, 0x40000000, 3, 2, 2, 1), (1, 10, 3, 2, 8, 0x10000000)):
        assert lib.lo_kernel_lmc_mv_workspace_bytes(*args) == 0, args


def test_gate_on_cpu_tensors():
    x = torch.rand(30, 3)
    Bt = torch.eye(2) + 0.1
    two = [kron(x, Bt), kron(x, Bt + 0.2, "matern52", 0.9)]
    assert _lmc_terms(two, check_device=False) == two
    four = two + [kron(x, Bt, "matern12"), kron(x, Bt, "matern32")]
    assert _lmc_terms(four, check_device=False) == four
    # what does not lower: one term (the single-term kind), five terms, other points, another T, a non-native factor, a
    # dense term mixed in
    assert _lmc_terms(two[:1], check_device=False) is None
    assert _lmc_terms(four + [kron(x, Bt)], check_device=False) is None
    assert _lmc_terms([two[0], kron(x.clone(), Bt)], check_device=False) is None
    assert _lmc_terms([two[0], kron(x, torch.eye(3))], check_device=False) is None
    other = KernelLinearOperator(x, x, lambda a, b, **kw: covariance.rbf(a, b, **kw), num_nonbatch_dimensions=NB,
                                 lengthscale=torch.ones(1, 3), outputscale=torch.tensor(1.0))
    assert _lmc_terms([two[0], KroneckerProductLinearOperator(other, DenseLinearOperator(Bt))], False) is None
    assert _lmc_terms([two[0], KroneckerProductLinearOperator(two[1].linear_ops[0], RootLinearOperator(torch.rand(2, 1)))],
                      False) is None
    assert _lmc_terms([two[0], two[1], DenseLinearOperator(torch.eye(60))], check_device=False) is None
    assert _lmc_terms([two[0], kron(x, torch.eye(9)), ], check_device=False) is None  # (T beyond LO_KERNEL_KRON_MAX_TASKS)
    # on CPU tensors the full gate refuses and nothing lowers: the sum, inside AddedDiag, and the SumKronecker of k1 + k2
    assert _lmc_terms(two) is None
    assert SumLinearOperator(*two)._kernel_descriptor() is None
    assert AddedDiagLinearOperator(SumLinearOperator(*two), DiagLinearOperator(torch.ones(60)))._kernel_descriptor() is None
    assert (two[0] + two[1])._kernel_descriptor() is None
    assert K._NATIVE_MATMUL_KERNEL_LMC is not None and all(
        1 <= q <= 4 and 1 <= t <= 8 and cls in (1, 2) for q, t, cls in K._NATIVE_MATMUL_KERNEL_LMC)


def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g46_kernel_lmc_{p}.npz"))


def lmc_op(p, t):
    ops = []
    for q, (family, _, _) in enumerate(CASES[p][0]):
        kern = KernelLinearOperator(t["x"], t["x"], covariance.FAMILIES[family], num_nonbatch_dimensions=NB,
                                    lengthscale=t[f"lengthscale{q}"], outputscale=t[f"outputscale{q}"])
        ops.append(KroneckerProductLinearOperator(kern, DenseLinearOperator(t[f"task{q}"])))
    return SumLinearOperator(*ops)


@pytest.mark.parametrize("p", list(CASES))
def test_fixtures_against_the_float64_dense_composition(p):
    """The fixtures load, hold every quantity, and their float64 values are those of the dense composition of the
    covariance functions; the CPU general path meets the product and the diagonal within the protocol's bound."""
    G = golden(p)
    terms, B, n, D, T, seed = CASES[p]
    t = {k: torch.from_numpy(v) for k, v in inputs(p).items()}
    t64 = {k: v.double() for k, v in t.items()}
    assert G["mv"].shape == (B, n * T, 4) and G["piv"].shape == (B, RANK) and G["L"].shape[-2:] in ((n * T, RANK), (RANK, n * T))
    quantities = ["mv", "diag", "solve", "iq", "L", "ld"] + sorted(grad_keys(p).values())
    assert len(quantities) == 7 + 3 * len(terms)
    for q in quantities:
        assert q in G.files and q + "_64" in G.files and float(G[q + "_err"]) < 2e-3, q
    for q in range(len(terms)):
        assert G[f"gB{q}"].shape == (B, T, T) and G[f"go{q}"].shape == (B,)
        assert G[f"gl{q}"].shape == (B, 1, D if terms[q][1] else 1)
    K64 = dense_lmc(p, t64, covariance.FAMILIES)
    A64 = K64 + torch.diag_embed(t64["noise"])
    assert rel((K64 @ t64["V"]).numpy(), G["mv_64"]) <= 1e-12
    assert rel(K64.diagonal(dim1=-1, dim2=-2).numpy(), G["diag_64"]) <= 1e-12
    assert rel(torch.linalg.solve(A64, t64["rhs"]).numpy(), G["solve_64"]) <= 1e-9
    assert rel(torch.logdet(A64).numpy(), G["ld_dense64"]) <= 1e-12
    op = lmc_op(p, t)
    assert _lmc_terms(list(op.linear_ops), check_device=False) is not None
    for q, val in (("mv", op @ t["V"]), ("diag", op.diagonal())):
        err, ref = rel(val.double().numpy(), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
        assert err <= REF_FACTOR * ref, (q, err, ref)
    # the diagonal is sum_q outputscale_q^2 (x) diag(B_q), index i T + t
    want = sum((t[f"outputscale{q}"] ** 2)[:, None, None] * t[f"task{q}"].diagonal(dim1=-1, dim2=-2)[:, None, :]
               for q in range(len(terms)))
    assert torch.allclose(op._diagonal(), want.expand(B, n, T).reshape(B, n * T))
