"""Every row of KernelLinearOperator's table of native variants through the operator's one product arm and one derivative
body, on the MI355X, at the smallest shapes at which the shared flattening can go wrong: an unbatched operator against
vectors of batch (2,) (the batch comes from the vector side), x1 with 5 points and x2 with 7 (rectangular, below one row
block), D = 2, T = 2, one column for the product, two vector pairs for the derivative, every parameter and both point
tensors asking for a gradient (the grad variant: the parameters only).

Bounds, as in tests/test_gpu_kernel_op.py, _grad.py, _task.py and _param.py: the error against the float64 dense
evaluation of the same covariance function (derivatives: float64 autograd through it) is at most REF_FACTOR = 4 times
the error of its float32 evaluation on the same inputs, floored at ERR_FLOOR = 1e-7.  The float64 variant, as in
tests/test_gpu_kernel_f64.py: the truth is the longdouble computation of tests/kernel_f64_cases.py, the reference the
float64 dense evaluation, the floor 2^-52.  The vectors are positive, so that the one-number gradients (outputscale,
alpha) are sums without cancellation and the reference's error is not a draw near zero."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import kernel_f64_cases as T  # noqa: E402
from make_golden_kernel_op import ERR_FLOOR, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd.operators import KernelLinearOperator  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF_FACTOR = 4.0
NB = {"outputscale": 0, "alpha": 0}
M, N, D, TASKS, PAIRS = 5, 7, 2, 2, 2
F32, F64 = torch.float32, torch.float64

# name -> (covariance function, element type, the kernel classes a product and a derivative must launch, those they may)
CASES = {
    "rbf": (covariance.rbf, F32, {"k_kernel_mv", "k_kernel_bil", "k_kernel_pgrad"},
            {"k_kernel_mv_reduce", "k_kernel_pgrad_reduce"}),
    "matern52_f64": (covariance.matern52, F64, {"k64_kernel_mv", "k64_kernel_bil", "k64_kernel_pgrad"},
                     {"k64_kernel_mv_reduce", "k64_kernel_pgrad_reduce"}),
    "rbf_grad": (covariance.rbf_grad, F32, {"k_kernel_grad_mv", "k_kernel_grad_bilinear"}, {"k_kernel_grad_mv_reduce"}),
    "matern32_task": (covariance.matern32_task, F32, {"k_kernel_task_mv", "k_kernel_task_bil", "k_kernel_task_pgrad"},
                      {"k_kernel_task_mv_reduce", "k_kernel_task_pgrad_reduce"}),
    "rq": (covariance.rq, F32, {"k_kparam_mv", "k_kparam_bil", "k_kparam_pgrad"},
           {"k_kparam_mv_reduce", "k_kparam_pgrad_reduce"}),
    "periodic": (covariance.periodic, F32, {"k_kparam_mv", "k_kparam_bil", "k_kparam_pgrad"},
                 {"k_kparam_mv_reduce", "k_kparam_pgrad_reduce"}),
}
FAMILY_KERNELS = set().union(*(must | may for _, _, must, may in CASES.values()))


class Counting:
    """covar_func with the native attributes of `fn` that counts its calls."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0
        self.native_family = fn.native_family
        if hasattr(fn, "native_outputs"):
            self.native_outputs = fn.native_outputs

    def __call__(self, *args, **kwargs):
        self.calls += 1
        return self.fn(*args, **kwargs)


def dev(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(DEV).to(dtype).contiguous()  # (a numpy scalar stays 0-dimensional)


def host(t):
    return t.detach().double().cpu().numpy()


def inputs(name):
    """(x1 [M, DX], x2 [N, DX], parameters, cols [2, N rows, 1], U [2, M rows, PAIRS], V [2, N rows, PAIRS]) in float64
    numpy, every value a float32 number."""
    g = np.random.Generator(np.random.PCG64(9700 + list(CASES).index(name)))
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    x1, x2 = f32(g.random((M, D))), f32(g.random((N, D)))
    params = {"lengthscale": f32(0.5 + 0.3 * g.random((1, D))), "outputscale": f32(0.8 + 0.7 * g.random(()))}
    rows = 1
    if name == "rbf_grad":
        rows = D + 1
    elif name == "matern32_task":
        x1 = np.concatenate((x1, g.integers(0, TASKS, (M, 1)).astype(np.float64)), -1)
        x2 = np.concatenate((x2, g.integers(0, TASKS, (N, 1)).astype(np.float64)), -1)
        root = g.standard_normal((TASKS, TASKS))
        params["task_covar"] = f32(root @ root.T + np.eye(TASKS))
    elif name == "rq":
        params["alpha"] = f32(0.5 + 2.5 * g.random(()))
    elif name == "periodic":
        params["period_length"] = f32(0.8 + 0.4 * g.random((1, 1)))  # (shared over D)
    cols = f32(g.standard_normal((2, N * rows, 1)))
    U, V = f32(0.5 + g.random((2, M * rows, PAIRS))), f32(0.5 + g.random((2, N * rows, PAIRS)))
    return x1, x2, params, cols, U, V


def dense(fn, dtype, x1, x2, params, cols, U, V, points):
    """{"product", "x1", "x2", parameter names} from the dense evaluation of fn in `dtype` on the device and autograd."""
    a, b = dev(x1, dtype).requires_grad_(points), dev(x2, dtype).requires_grad_(points)
    leaves = {k: dev(v, dtype).requires_grad_(True) for k, v in params.items()}
    Kd = fn(a, b, **leaves)
    out = {"product": host(Kd @ dev(cols, dtype))}
    (dev(U, dtype) * (Kd @ dev(V, dtype))).sum().backward()
    out.update({k: host(v.grad) for k, v in leaves.items()})
    if points:
        out.update(x1=host(a.grad), x2=host(b.grad))
    return out


def longdouble_truth(x1, x2, params, cols, U, V):
    """The same quantities for matern52 from tests/kernel_f64_cases.py, the members of the vectors' batch summed."""
    rep = lambda a: np.broadcast_to(a, (2, *a.shape))  # noqa: E731
    theta = T.theta_ld(params["lengthscale"], params["outputscale"], 2, D)
    d_ls, d_os = T.theta_to_params(theta, T.g_theta_ld("matern52", rep(x1), rep(x2), theta, U, V), ard=True)
    return {"product": T.dense_ld("matern52", rep(x1), rep(x2), theta) @ cols.astype(T.LD),
            "lengthscale": d_ls.sum(0), "outputscale": d_os.sum(0),
            "x1": T.g_x1_ld("matern52", rep(x1), rep(x2), theta, U, V).sum(0),
            "x2": T.g_x1_ld("matern52", rep(x2), rep(x1), theta, V, U).sum(0)}


@pytest.mark.parametrize("name", list(CASES))
def test_variant_through_the_shared_product_and_derivative(name):
    fn, dtype, must, may = CASES[name]
    x1, x2, params, cols, U, V = inputs(name)
    points = name != "rbf_grad"
    ref = dense(fn, dtype, x1, x2, params, cols, U, V, points)
    if dtype == F64:
        truth, floor, err_of = longdouble_truth(x1, x2, params, cols, U, V), T.FLOOR, T.rel
    else:
        truth, floor, err_of = dense(fn, F64, x1, x2, params, cols, U, V, points), ERR_FLOOR, rel
    covar = Counting(fn)
    tensors = {k: dev(v, dtype).requires_grad_(True) for k, v in params.items()}
    op = KernelLinearOperator(dev(x1, dtype).requires_grad_(points), dev(x2, dtype).requires_grad_(points), covar,
                              num_outputs_per_input=(D + 1, D + 1) if name == "rbf_grad" else (1, 1),
                              num_nonbatch_dimensions=NB, **tensors)
    assert op.batch_shape == torch.Size([])
    rhs, tU, tV = dev(cols, dtype), dev(U, dtype), dev(V, dtype)
    other = rhs.to(F64 if dtype == F32 else F32)
    _hip.prof_enable(True)
    try:
        _hip.prof_report()
        y = op._matmul(rhs)
        grads = op._bilinear_derivative(tU, tV)
        torch.cuda.synchronize()
        launched = set(_hip.prof_report())
        assert covar.calls == 0
        try:  # a right-hand side of the other float type: the general path (whose matmul torch may refuse for the types)
            op._matmul(other)
        except RuntimeError:
            pass
        torch.cuda.synchronize()
        assert covar.calls == 1
        assert not FAMILY_KERNELS & set(_hip.prof_report())
    finally:
        _hip.prof_enable(False)
    assert must <= launched <= must | may, launched
    got = dict(zip(("x1", "x2", *op._differentiable_kwargs), grads), product=y)
    assert y.shape == ref["product"].shape and y.dtype == dtype
    if not points:
        assert got.pop("x1") is None and got.pop("x2") is None
    assert set(got) == set(truth)
    for what, value in got.items():
        assert tuple(value.shape) == truth[what].shape and bool(torch.isfinite(value).all()), what
        err, ref_err = err_of(host(value), truth[what]), max(err_of(ref[what], truth[what]), floor)
        print(f"kernel variant {name} {what}: err {err:.3e} reference {ref_err:.3e} ratio {err / ref_err:.2f}")
        assert err <= REF_FACTOR * ref_err, (name, what, err, ref_err)
