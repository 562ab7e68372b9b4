"""The host side of the float64 many-column kernel derivatives (csrc/lo_kernel_bil_wide_f64.hip, ABI 45) without a GPU: the
version, the four symbols and the workspace sizers, which lay the partials out exactly as the sizers of
lo_kernel_bilinear_f64 and lo_kernel_points_grad_f64 do."""
import pytest

from linear_operator_amd import _hip

STEMS = ("lo_kernel_bilinear", "lo_kernel_points_grad")


def test_abi_and_symbols():
    lib = _hip.load()
    assert _hip.ABI_VERSION >= 45 and lib.lo_abi_version() == _hip.ABI_VERSION
    assert {s + e for s in STEMS for e in ("_wide_f64", "_wide_f64_workspace_bytes")} <= set(_hip.EXPORTS)


# (B, M, N, D, t, split): js = 1 (one tile of points; B ceil(M / 256) >= 512) and js > 1
@pytest.mark.parametrize("shape", [(1, 300, 100, 3, 17, False), (512, 33, 129, 3, 17, False), (1, 300, 300, 3, 17, True),
                                   (3, 1013, 700, 8, 65, True), (1, 16384, 16384, 32, 33, True)])
@pytest.mark.parametrize("stem", STEMS)
def test_sizers_equal_the_plain_float64_sizers(stem, shape):
    lib, (B, M, N, D, t, split) = _hip.load(), shape
    wide, plain = getattr(lib, stem + "_wide_f64_workspace_bytes"), getattr(lib, stem + "_f64_workspace_bytes")
    need = wide(B, M, N, D, t)
    assert need == plain(B, M, N, D, t) and need >= 256
    if stem == "lo_kernel_points_grad":  # (the hyperparameters always keep a partial per workgroup)
        assert (need > 256) == split
    assert wide(B, M, N, 33, t) == 0 and wide(B, 0, N, D, t) == 0
