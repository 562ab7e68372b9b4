"""The host side of csrc/lo_kernel_kinds_wide.hip (ABI 46) without a GPU: the version, the four symbols and the workspace
sizers, which lay the split-j partials out exactly as the one-column sizers of the two kinds do."""
import pytest

from linear_operator_amd import _hip


def test_abi_and_symbols():
    lib = _hip.load()
    assert _hip.ABI_VERSION >= 46 and lib.lo_abi_version() == _hip.ABI_VERSION
    assert {"lo_kernel_param_mv_wide_f32", "lo_kernel_param_mv_wide_workspace_bytes", "lo_kernel_sm_mv_wide_f32",
            "lo_kernel_sm_mv_wide_workspace_bytes"} <= set(_hip.EXPORTS)


# (B, M, N, D, c, split): js = 1 (one tile of points; B ceil(M / 256) >= 512) and js > 1
@pytest.mark.parametrize("shape", [(1, 300, 100, 3, 17, False), (512, 33, 129, 3, 17, False), (1, 300, 300, 3, 17, True),
                                   (3, 1013, 700, 8, 65, True), (1, 16384, 16384, 16, 33, True)])
def test_sizers_equal_the_one_column_sizers(shape):
    lib, (B, M, N, D, c, split) = _hip.load(), shape
    need = lib.lo_kernel_param_mv_wide_workspace_bytes(B, M, N, D, c)
    assert need == lib.lo_kernel_param_mv_workspace_bytes(B, M, N, D, c) and (need > 256) == split
    need = lib.lo_kernel_sm_mv_wide_workspace_bytes(B, M, N, D, 4, c)
    assert need == lib.lo_kernel_sm_mv_workspace_bytes(B, M, N, D, 4, c) and (need > 256) == split
    # beyond the kinds' limits: D = 33; D = 17, Q = 17
    assert lib.lo_kernel_param_mv_wide_workspace_bytes(B, M, N, 33, c) == 0
    assert lib.lo_kernel_sm_mv_wide_workspace_bytes(B, M, N, 17, 4, c) == 0
    assert lib.lo_kernel_sm_mv_wide_workspace_bytes(B, M, N, D, 17, c) == 0
