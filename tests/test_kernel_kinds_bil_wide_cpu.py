"""The host side of csrc/lo_kernel_kinds_bil_wide.hip (ABI 47) without a GPU: the version, the eight symbols and the
workspace sizers, which lay the partials out exactly as the sizers of the plain derivative entries of the two kinds do."""
import pytest

from linear_operator_amd import _hip

STEMS = ["lo_kernel_param_bilinear", "lo_kernel_param_points_grad", "lo_kernel_sm_bilinear", "lo_kernel_sm_points_grad"]


def test_abi_and_symbols():
    lib = _hip.load()
    assert _hip.ABI_VERSION >= 47 and lib.lo_abi_version() == _hip.ABI_VERSION
    assert {s + e for s in STEMS for e in ("_wide_f32", "_wide_workspace_bytes")} <= set(_hip.EXPORTS)


# (B, M, N, D, t): an unsplit shape (B ceil(M / 256) >= 512) and a split one
@pytest.mark.parametrize("shape", [(512, 33, 129, 3, 17), (3, 1013, 700, 8, 65)])
@pytest.mark.parametrize("stem", STEMS)
def test_sizers_equal_their_twins(stem, shape):
    lib, (B, M, N, D, t) = _hip.load(), shape
    wide, plain = getattr(lib, stem + "_wide_workspace_bytes"), getattr(lib, stem + "_workspace_bytes")
    if "_sm_" in stem:
        assert wide(B, M, N, D, 4, t) == plain(B, M, N, D, 4, t) >= 256
        assert wide(B, M, N, 17, 4, t) == 0 and wide(B, M, N, D, 17, t) == 0  # beyond the kind's limits
    else:
        assert wide(B, M, N, D, t) == plain(B, M, N, D, t) >= 256
        assert wide(B, M, N, 33, t) == 0
