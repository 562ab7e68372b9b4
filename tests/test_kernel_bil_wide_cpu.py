"""The host side of the many-column kernel derivatives (csrc/lo_kernel_bil_wide.hip, ABI 43) without a GPU: the version,
the four symbols and the workspace sizers, which lay the partials out exactly as their plain twins do."""
import pytest

from linear_operator_amd import _hip

STEMS = ("lo_kernel_bilinear", "lo_kernel_points_grad")


def test_abi_and_symbols():
    lib = _hip.load()
    assert _hip.ABI_VERSION >= 43 and lib.lo_abi_version() == _hip.ABI_VERSION
    assert {s + tail for s in STEMS for tail in ("_wide_f32", "_wide_workspace_bytes")} <= set(_hip.EXPORTS)


# (B, M, N, D, t): js = 1 (B ceil(M / 256) >= 512) and js > 1
@pytest.mark.parametrize("shape", [(512, 33, 129, 3, 17), (1, 300, 300, 3, 17), (3, 1013, 700, 8, 65)])
@pytest.mark.parametrize("stem", STEMS)
def test_sizers_equal_their_plain_twins(stem, shape):
    lib, (B, M, N, D, t) = _hip.load(), shape
    need = getattr(lib, stem + "_wide_workspace_bytes")(B, M, N, D, t)
    assert need == getattr(lib, stem + "_workspace_bytes")(B, M, N, D, t) and need >= 256
    assert getattr(lib, stem + "_wide_workspace_bytes")(B, M, N, 33, t) == 0
