"""The task-indexed ("Hadamard") multitask kernels without a GPU: covariance.*_task against a hand-written float64 double
loop, the binding of ABI 34 (symbols, constants, the host-side sizers), the gate `_native_task_refusal` decided on CPU
tensors through its `check_device=False` form (with `_native_refusal` answering what it always did, so the Sum and
Kronecker fusion gates stay out), and the general path on the CPU against the dense matrix."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_task import CASES, inputs  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, SumLinearOperator)

NB = {"outputscale": 0}
F8 = torch.float64


def points(g, batch, n, D, T, dtype=F8):
    """[*batch, n, D + 1]: D coordinates, then the task id as a float."""
    ids = torch.randint(0, T, (*batch, n, 1), generator=g).to(dtype)
    return torch.cat((torch.rand(*batch, n, D, generator=g, dtype=dtype), ids), -1)


def task_table(g, batch, T, dtype=F8):
    a = torch.rand(*batch, T, T, generator=g, dtype=dtype)
    return a @ a.mT + torch.diag_embed(1.0 + torch.arange(T, dtype=dtype).expand(*batch, T))


def task_op(x, x2=None, fn=covariance.rbf_task, dtype=torch.float32, T=3, ls=None, Bt=None, nb=NB, **extra):
    D = x.shape[-1] - 1
    ls = torch.linspace(0.5, 0.9, max(D, 1), dtype=dtype).reshape(1, max(D, 1)) if ls is None else ls
    Bt = (torch.eye(T, dtype=dtype) + 0.2) if Bt is None else Bt
    return KernelLinearOperator(x, x if x2 is None else x2, fn, num_nonbatch_dimensions=nb, lengthscale=ls,
                                outputscale=torch.tensor(1.1, dtype=dtype), task_covar=Bt, **extra)


G_OF_R = {
    "rbf": lambda r: math.exp(-0.5 * r * r),
    "matern12": lambda r: math.exp(-r),
    "matern32": lambda r: (1.0 + math.sqrt(3.0) * r) * math.exp(-math.sqrt(3.0) * r),
    "matern52": lambda r: (1.0 + math.sqrt(5.0) * r + 5.0 * r * r / 3.0) * math.exp(-math.sqrt(5.0) * r),
}


@pytest.mark.parametrize("family", list(G_OF_R))
@pytest.mark.parametrize("shared", [False, True])
def test_task_functions_are_the_double_loop(family, shared):
    """K_ij = os^2 g(|(x_i - x_j) / l|) Bt[t_i, t_j], entry by entry in float64, n = 5, a non-symmetric table (the lookup
    is [t_i, t_j], not its transpose), rectangular and batched."""
    g = torch.Generator().manual_seed(43)
    n, m, D, T = 5, 4, 3, 3
    fn = covariance.TASK_FAMILIES[family + "_task"]
    x1, x2 = points(g, (2,), n, D, T), points(g, (2,), m, D, T)
    ls = torch.rand(2, 1, 1 if shared else D, generator=g, dtype=F8) + 0.5
    os_ = torch.rand(2, generator=g, dtype=F8) + 0.5
    Bt = torch.rand(2, T, T, generator=g, dtype=F8)
    assert not torch.allclose(Bt, Bt.mT)
    got = fn(x1, x2, ls, os_, Bt)
    assert got.shape == (2, n, m) and got.dtype == F8
    for b in range(2):
        for i in range(n):
            for j in range(m):
                r = math.sqrt(sum(((float(x1[b, i, k]) - float(x2[b, j, k])) / float(ls[b, 0, 0 if shared else k])) ** 2
                                  for k in range(D)))
                want = float(os_[b]) ** 2 * G_OF_R[family](r) * float(Bt[b, int(x1[b, i, D]), int(x2[b, j, D])])
                assert abs(float(got[b, i, j]) - want) <= 1e-14 * max(1.0, abs(want)), (b, i, j)
    assert fn(x1.float(), x2.float(), ls.float(), os_.float(), Bt.float()).dtype == torch.float32


def test_task_functions_survive_the_pairs_as_a_batch_dimension_and_differentiate():
    """The call pattern of `_diagonal` and `_get_indices` (x as [n, *b, 1, D + 1], the parameters with one more leading
    dimension); the gradients of every parameter flow and the task column's gradient is zero."""
    g = torch.Generator().manual_seed(44)
    x = points(g, (2,), 5, 3, 3).requires_grad_(True)
    ls = (torch.rand(2, 1, 3, generator=g, dtype=F8) + 0.5).requires_grad_(True)
    os_ = (torch.rand(2, generator=g, dtype=F8) + 0.5).requires_grad_(True)
    Bt = task_table(g, (2,), 3).requires_grad_(True)
    a = x.movedim(-2, 0).unsqueeze(-2)
    blocks = covariance.matern52_task(a, a, ls.unsqueeze(0), os_.unsqueeze(0), Bt.unsqueeze(0))
    full = covariance.matern52_task(x, x, ls, os_, Bt)
    assert blocks.shape == (5, 2, 1, 1)
    assert torch.allclose(blocks[..., 0, 0].movedim(0, -1), full.diagonal(dim1=-2, dim2=-1), atol=1e-15)
    (full * torch.rand(2, 5, 5, generator=g, dtype=F8)).sum().backward()
    assert all(bool(t.grad.abs().sum() > 0) for t in (ls, os_, Bt))
    assert bool(x.grad[..., :3].abs().sum() > 0) and not x.grad[..., 3].any()


def test_attributes_and_the_family_dicts():
    names = ("rbf", "matern12", "matern32", "matern52")
    assert list(covariance.TASK_FAMILIES) == [n + "_task" for n in names]
    for n in names:
        f = covariance.TASK_FAMILIES[n + "_task"]
        assert f is getattr(covariance, n + "_task") and f.__name__ == n + "_task"
        assert f.native_family == covariance.FAMILIES[n].native_family and f.native_outputs == "task"
    assert not set(covariance.TASK_FAMILIES) & (set(covariance.FAMILIES) | set(covariance.GRAD_FAMILIES))
    assert all(getattr(f, "native_outputs", None) is None for f in covariance.FAMILIES.values())


def test_binding_of_abi_34():
    assert _hip.LO_OP_KERNEL_TASK_DIAG == 15 and _hip.LO_KERNEL_TASK_MAX_TASKS == 8 and _hip.ABI_VERSION >= 34
    for name, nargs in (("lo_kernel_task_mv_workspace_bytes", 6), ("lo_kernel_task_mv_f32", 18),
                        ("lo_kernel_task_bilinear_workspace_bytes", 6), ("lo_kernel_task_bilinear_f32", 18),
                        ("lo_kernel_task_points_grad_workspace_bytes", 6), ("lo_kernel_task_points_grad_f32", 17)):
        assert name in _hip.EXPORTS and len(_hip._PROTOTYPES[name][1]) == nargs
    for name in ("kernel_task_mv", "kernel_task_bilinear", "kernel_task_points_grad", "kernel_task_diag_descriptor"):
        assert callable(getattr(K, name))
    lib = _hip.load()  # (raises when the library does not export a symbol of the table; the sizers are host code)
    assert lib.lo_abi_version() == _hip.ABI_VERSION
    # the struct of the kind: no new member, T rides in nterms, the family in n2, R counts the coordinates
    s = K.OperatorDescriptor(_hip.LO_OP_KERNEL_TASK_DIAG, 2, 40, R=3, n2=2, kernel_terms=4).c_struct()
    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (15, 4, 2, 3, 40)


def split_count(B, M, N):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-M // 256), -(-N // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return rb, -(-N // jchunk)


@pytest.mark.parametrize("B,M,N,D,T,c", [(512, 40, 40, 2, 2, 2), (1, 1, 1, 1, 1, 1), (1, 257, 300, 3, 3, 17),
                                         (3, 130, 70, 31, 8, 1), (1, 16384, 16384, 4, 4, 1), (8, 4096, 4096, 16, 8, 17)])
def test_sizers_are_the_closed_form_of_the_layouts(B, M, N, D, T, c):
    lib = _hip.load()
    rb, js = split_count(B, M, N)
    split = js > 1
    assert lib.lo_kernel_task_mv_workspace_bytes(B, M, N, D, T, c) == 256 + (4 * js * B * M * c if split else 0)
    assert lib.lo_kernel_task_points_grad_workspace_bytes(B, M, N, D, T, c) == 256 + (4 * js * B * M * (D + 1) if split else 0)
    DP = 4 if D <= 4 else (8 if D <= 8 else (16 if D <= 16 else 32))
    assert lib.lo_kernel_task_bilinear_workspace_bytes(B, M, N, D, T, c) == 256 + 4 * B * rb * js * (DP + T * T)


def test_sizers_refuse_what_the_entry_points_refuse():
    lib = _hip.load()
    sizers = (lib.lo_kernel_task_mv_workspace_bytes, lib.lo_kernel_task_bilinear_workspace_bytes,
              lib.lo_kernel_task_points_grad_workspace_bytes)
    for args in ((1, 10, 10, 32, 2, 1), (1, 10, 10, 3, 9, 1), (0, 10, 10, 3, 2, 1), (1, 0, 10, 3, 2, 1),
                 (1, 10, 0, 3, 2, 1), (1, 10, 10, 0, 2, 1), (1, 10, 10, 3, 0, 1), (1, 10, 10, 3, 2, 0),
                 (65536, 10, 10, 3, 2, 1)):
        for sizer in sizers:
            assert sizer(*args) == 0, args  # (D + 1 = 33, T = 9, zero sizes, too many members)
    for sizer in sizers:
        assert sizer(1, 10, 10, 31, 8, 1) >= 256


def test_every_branch_of_the_gate():
    g = torch.Generator().manual_seed(45)
    f4 = torch.float32
    x = points(g, (), 20, 3, 3, f4)
    ok = task_op(x)
    assert ok._native_task_refusal(check_device=False) is None
    assert "device" in ok._native_task_refusal() and not ok._is_native_task()  # (CPU tensors)
    assert ok._kernel_descriptor() is None
    for D in (1, 31):
        assert task_op(points(g, (), 20, D, 3, f4))._native_task_refusal(check_device=False) is None
    assert task_op(x, T=1)._native_task_refusal(check_device=False) is None
    assert task_op(x, T=8)._native_task_refusal(check_device=False) is None
    assert task_op(x, ls=torch.full((1, 1), 0.7))._native_task_refusal(check_device=False) is None  # (a shared lengthscale)
    xb = points(g, (2,), 20, 3, 3, f4)
    batched = KernelLinearOperator(xb, xb, covariance.matern32_task, num_nonbatch_dimensions=NB,
                                   lengthscale=torch.full((2, 1, 3), 0.7), outputscale=torch.ones(2),
                                   task_covar=task_table(g, (2,), 3, f4))
    assert batched._native_task_refusal(check_device=False) is None

    def refusal(op):
        return op._native_task_refusal(check_device=False)

    assert "native_outputs" in refusal(KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB,
                                                            lengthscale=torch.ones(1, 4), outputscale=torch.tensor(1.0)))

    def no_family(x1, x2, **params):
        return covariance.rbf_task(x1, x2, **params)

    no_family.native_outputs = "task"
    assert "native_family" in refusal(task_op(x, fn=no_family))
    assert "one output per input" in refusal(task_op(x, num_outputs_per_input=(2, 2)))
    assert "parameters other than" in refusal(task_op(x, extra=torch.ones(1)))
    assert "parameters other than" in refusal(task_op(x, flag=True))
    assert "parameters other than" in refusal(KernelLinearOperator(
        x, x, covariance.rbf_task, num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 3),
        outputscale=torch.tensor(1.0)))
    assert "D = 32" in refusal(task_op(points(g, (), 20, 32, 3, f4)))
    assert "D = 0" in refusal(task_op(torch.zeros(20, 1)))
    assert "D = " in refusal(task_op(x, x2=points(g, (), 20, 4, 3, f4), ls=torch.ones(1, 1)))
    assert "lengthscale" in refusal(task_op(x, ls=torch.ones(1, 2)))
    assert "lengthscale" in refusal(task_op(x, ls=torch.ones(3), nb={"outputscale": 0, "lengthscale": 1}))
    assert "outputscale" in refusal(KernelLinearOperator(x, x, covariance.rbf_task, lengthscale=torch.ones(1, 3),
                                                         outputscale=torch.ones(1, 1), task_covar=torch.eye(3)))
    assert "task_covar" in refusal(task_op(x, Bt=torch.ones(3, 2)))
    assert "task_covar" in refusal(task_op(x, Bt=torch.ones(3), nb={"outputscale": 0, "task_covar": 1}))
    assert "T = 9" in refusal(task_op(x, T=9))
    assert "float32" in refusal(task_op(x.double(), dtype=F8))
    assert "float32" in refusal(task_op(x, Bt=torch.eye(3, dtype=F8)))


def test_the_other_gates_stay_out():
    """`_native_refusal` (and its float64 twin) keep answering "parameters other than lengthscale and outputscale" for a
    task operator, so the fused kernel sum and the Kronecker multitask kind never take one; the task gate refuses the plain
    families."""
    from linear_operator_amd.operators.sum_linear_operator import _kernel_group_pair

    g = torch.Generator().manual_seed(46)
    x = points(g, (), 20, 3, 3, torch.float32)
    op = task_op(x)
    why = "parameters other than lengthscale and outputscale"
    assert op._native_refusal(check_device=False) == why and op._native_refusal() == why
    assert task_op(x.double(), dtype=F8)._native_f64_refusal(check_device=False) == why
    assert "native_outputs" in op._native_grad_refusal(check_device=False)
    assert not op._is_native() and not op._is_native_f64() and not op._is_native_grad()
    plain = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 4),
                                 outputscale=torch.tensor(1.0))
    assert _kernel_group_pair([op, op]) is None and _kernel_group_pair([plain, op]) is None
    assert SumLinearOperator(op, op)._kernel_descriptor() is None
    kron = KroneckerProductLinearOperator(op, DenseLinearOperator(torch.eye(2)))
    assert kron._kernel_kron_refusal(check_device=False) is not None and kron._kernel_descriptor() is None


@pytest.mark.parametrize("p", list(CASES))
def test_general_path_on_the_cpu_is_the_dense_matrix(p):
    """The fixtures' inputs in float64 on the CPU: matmul, transpose, diagonal, slicing,
    single entries and the gradients of inv_quad against the dense matrix; in float32 the diagonal is the gather."""
    family, B, n, D, T, ard, seed = CASES[p]
    fn = covariance.TASK_FAMILIES[family + "_task"]
    t = {k: torch.from_numpy(v).to(F8) for k, v in inputs(p).items()}
    calls = []

    def counted(x1, x2, **params):
        calls.append((x1.shape[-2], x2.shape[-2]))
        return fn(x1, x2, **params)

    counted.native_family, counted.native_outputs = fn.native_family, fn.native_outputs
    op = KernelLinearOperator(t["x"], t["x"], counted, num_nonbatch_dimensions=NB, lengthscale=t["lengthscale"],
                              outputscale=t["outputscale"], task_covar=t["task_covar"])
    dense = fn(t["x"], t["x"], t["lengthscale"], t["outputscale"], t["task_covar"])
    assert op.shape == (B, n, n)
    assert torch.allclose(op @ t["V"], dense @ t["V"], rtol=1e-13, atol=1e-13)
    assert torch.allclose(op.mT @ t["V"], dense.mT @ t["V"], rtol=1e-13, atol=1e-13)
    calls.clear()
    assert torch.allclose(op.diagonal(), dense.diagonal(dim1=-2, dim2=-1), rtol=1e-14, atol=0)
    assert calls == [(1, 1)]  # (float64 is outside the gate: the general path, one 1 x 1 matrix per point)
    calls.clear()
    x32 = t["x"].float()
    f32 = KernelLinearOperator(x32, x32, counted, num_nonbatch_dimensions=NB,
                               lengthscale=t["lengthscale"].float(), outputscale=t["outputscale"].float(),
                               task_covar=t["task_covar"].float())
    assert torch.allclose(f32.diagonal().double(), dense.diagonal(dim1=-2, dim2=-1), rtol=1e-6) and not calls
    sub = op[..., 3:40, 17:90]
    assert isinstance(sub, KernelLinearOperator) and sub.shape == (B, 37, 73)
    assert torch.allclose(sub.to_dense(), dense[..., 3:40, 17:90], rtol=1e-14, atol=0)
    assert calls[-1] == (37, 73)  # (only what is requested)
    rows, cols = torch.tensor([0, 5, n - 1]), torch.tensor([2, 5, 0])
    bidx = torch.zeros(3, dtype=torch.long)
    assert torch.allclose(op._get_indices(rows, cols, bidx), dense[bidx, rows, cols], rtol=1e-14, atol=0)
    assert calls[-1] == (1, 1)

    def leaves():
        out = dict(t)
        for k in ("x", "lengthscale", "outputscale", "task_covar"):
            out[k] = t[k].clone().requires_grad_(True)
        return out

    a, b = leaves(), leaves()
    A = AddedDiagLinearOperator(
        KernelLinearOperator(a["x"], a["x"], fn, num_nonbatch_dimensions=NB, lengthscale=a["lengthscale"],
                             outputscale=a["outputscale"], task_covar=a["task_covar"]), DiagLinearOperator(a["noise"]))
    from linear_operator_amd import settings

    with settings.fast_computations(solves=False, log_prob=False, covar_root_decomposition=False):
        A.inv_quad(a["rhs"]).sum().backward()
    k = fn(b["x"], b["x"], b["lengthscale"], b["outputscale"], b["task_covar"]) + torch.diag_embed(b["noise"])
    (b["rhs"] * torch.linalg.solve(k, b["rhs"])).sum().backward()
    for name in ("x", "lengthscale", "outputscale", "task_covar"):
        err = float((a[name].grad - b[name].grad).norm() / b[name].grad.norm())
        assert err < 1e-9, (name, err)
    assert not a["x"].grad[..., D].any()
    assert np.isfinite(float(dense.sum()))
