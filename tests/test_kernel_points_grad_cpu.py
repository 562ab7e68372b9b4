"""The points' gradient of KernelLinearOperator without a GPU: the binding of ABI 27 (lo_kernel_points_grad_f32 and its
sizer, which is host code), kernels.kernel_points_grad, and the removal of the chunked autograd path."""
import inspect

import torch

from linear_operator_amd import _hip
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import KernelLinearOperator, kernel_linear_operator

NAMES = ("lo_kernel_points_grad_workspace_bytes", "lo_kernel_points_grad_f32")


def column_splits(B, M, N):
    """ko_shape of csrc/lo_kernel_op.hip restated: the workgroups a member's columns are split over."""
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    wgs, tiles, js = ceil(M, 256) * B, ceil(N, 128), 1
    if wgs < 512:
        js = min(tiles, ceil(512, wgs), 64)
    jchunk = ceil(tiles, js) * 128
    return ceil(N, jchunk)


def test_binding_of_abi_27():
    assert _hip.ABI_VERSION >= 27
    for name in NAMES:
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["lo_kernel_points_grad_workspace_bytes"][1]) == 5
    assert len(_hip._PROTOTYPES["lo_kernel_points_grad_f32"][1]) == 15
    assert _hip.load().lo_abi_version() == _hip.ABI_VERSION


def test_sizer_measures_the_partials_of_a_split_member():
    lib = _hip.load()
    B, M, N, D, t = 1, 1013, 1013, 8, 3
    js = column_splits(B, M, N)
    assert js == 8
    need = lib.lo_kernel_points_grad_workspace_bytes(B, M, N, D, t)
    assert need > 0 and need >= 4 * js * B * M * D
    assert need < 4 * js * B * M * D + 1024  # (the partials and the tail, nothing else)
    # a rectangular pair and its transposed problem are sized by their own rows and their own splits
    assert column_splits(1, 77, 130) == 2 and column_splits(1, 130, 77) == 1
    assert lib.lo_kernel_points_grad_workspace_bytes(1, 77, 130, 3, 1) >= 4 * 2 * 77 * 3
    assert lib.lo_kernel_points_grad_workspace_bytes(1, 130, 77, 3, 1) == 256  # (one split: no partials, the tail)


def test_sizer_without_a_split_and_outside_the_gate():
    lib = _hip.load()
    assert column_splits(512, 40, 40) == 1
    assert lib.lo_kernel_points_grad_workspace_bytes(512, 40, 40, 2, 2) == 256  # (nothing but the tail)
    assert lib.lo_kernel_points_grad_workspace_bytes(1, 10, 10, 33, 1) == 0
    assert lib.lo_kernel_points_grad_workspace_bytes(0, 10, 10, 3, 1) == 0
    assert lib.lo_kernel_points_grad_workspace_bytes(1, 10, 10, 3, 0) == 0


def test_python_layers():
    assert callable(K.kernel_points_grad)
    assert list(inspect.signature(K.kernel_points_grad).parameters) == ["x1", "x2", "theta", "family", "U", "V"]
    assert not hasattr(KernelLinearOperator, "_points_derivative_chunked")
    assert not hasattr(kernel_linear_operator, "MAX_DENSE_CHUNK_BYTES")
    # the points' gradients come from the wrapper the variant's table row names, called by _bilinear_derivative_native
    plain = next(v for v in kernel_linear_operator.VARIANTS if v.tag is None and v.dtype == torch.float32)
    assert plain.points_grad == "kernel_points_grad"
    assert "getattr(K, v.points_grad)" in inspect.getsource(KernelLinearOperator._bilinear_derivative_native)
