"""The host side of the float64 many-column kernel product (csrc/lo_kernel_mv_wide_f64.hip, ABI 44) without a GPU: the
version, the two symbols and the workspace sizer, which lays the split-j partials out exactly as
lo_kernel_mv_f64_workspace_bytes does."""
import pytest

from linear_operator_amd import _hip


def test_abi_and_symbols():
    lib = _hip.load()
    assert _hip.ABI_VERSION >= 44 and lib.lo_abi_version() == _hip.ABI_VERSION
    assert {"lo_kernel_mv_wide_f64", "lo_kernel_mv_wide_f64_workspace_bytes"} <= set(_hip.EXPORTS)


# (B, M, N, D, c, split): js = 1 (one tile of points; B ceil(M / 256) >= 512) and js > 1
@pytest.mark.parametrize("shape", [(1, 300, 100, 3, 17, False), (512, 33, 129, 3, 17, False), (1, 300, 300, 3, 17, True),
                                   (3, 1013, 700, 8, 65, True), (1, 16384, 16384, 32, 33, True)])
def test_sizer_equals_the_product_sizer(shape):
    lib, (B, M, N, D, c, split) = _hip.load(), shape
    need = lib.lo_kernel_mv_wide_f64_workspace_bytes(B, M, N, D, c)
    assert need == lib.lo_kernel_mv_f64_workspace_bytes(B, M, N, D, c) and (need > 256) == split
    assert lib.lo_kernel_mv_wide_f64_workspace_bytes(B, M, N, 33, c) == 0
    assert lib.lo_kernel_mv_wide_f64_workspace_bytes(B, 0, N, D, c) == 0
