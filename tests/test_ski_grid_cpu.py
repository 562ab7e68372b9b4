"""SKI on a 2-D / 3-D grid without a GPU: the ABI pieces of LO_OP_SKI_GRID_DIAG (include/lo_amd.h against _hip.py), the
routing on the CPU / in float64, and the golden pinned to the reference's ordering of the Kronecker index."""
import ctypes
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_ski_grid import grid_inputs, kron_dense64, w_dense64  # noqa: E402

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    InterpolatedLinearOperator, KroneckerProductLinearOperator, ToeplitzLinearOperator)

X = grid_inputs()
G = np.load(os.path.join(HERE, "golden", "g35_ski_grid.npz"))
HDR = open(os.path.join(ROOT, "include", "lo_amd.h")).read()


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None or not t.dtype.is_floating_point else t.to(dtype)


def operator(cols, p, dtype=None, separate=False):
    base = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(T(X[c], dtype)) for c in cols])
    li, lv = X[p + "_li"], X[p + "_lv"]
    ri, rv = (X[p + "_ri"], X[p + "_rv"]) if separate else (li, lv)
    return InterpolatedLinearOperator(base, T(li), T(lv, dtype), T(ri), T(rv, dtype))


def test_abi_constants_and_interp_desc_tail():
    assert _hip.ABI_VERSION >= 23
    assert _hip.LO_OP_SKI_GRID_DIAG == 9
    for name in ("LO_OP_SKI_GRID_DIAG", "LO_SKI_GRID_MAX_AXIS", "LO_SKI_GRID_MAX_M"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", HDR).group(1)) == getattr(_hip, name)
    assert _hip.LO_SKI_GRID_MAX_AXIS == 1024 and _hip.LO_SKI_GRID_MAX_M == 1 << 22
    fields = dict(_hip.InterpDesc._fields_)
    assert fields["grid_ndim"] is ctypes.c_int32 and fields["grid_reserved"] is ctypes.c_int32
    assert ctypes.sizeof(fields["grid_m"]) == 24
    # appended behind the ABI-16 members: their offsets are unchanged
    assert _hip.InterpDesc.right_plan.offset == 32 and _hip.InterpDesc.grid_ndim.offset == 40
    assert _hip.InterpDesc.grid_m.offset == 48 and ctypes.sizeof(_hip.InterpDesc) == 72
    assert ctypes.sizeof(_hip.OpDesc) == 80 and _hip.OpDesc.terms.offset == 72


def test_header_declares_the_new_exports():
    for name in ("lo_toeplitz_kron_mv_f32", "lo_toeplitz_kron_workspace_bytes"):
        assert re.search(rf"\b{name}\s*\(", HDR), name
        assert name in _hip.EXPORTS


def test_descriptor_is_none_on_cpu_and_in_float64():
    assert operator(("g2_c1", "g2_c2"), "g2b1")._kernel_descriptor() is None
    assert operator(("g2_c1", "g2_c2"), "g2b1", torch.float64)._kernel_descriptor() is None
    assert operator(("g3_c1", "g3_c2", "g3_c3"), "g3")._kernel_descriptor() is None


def test_composition_reproduces_the_golden_matmul():
    """The operator's composed `_matmul` on the CPU against the reference's: pins the fixture (and the input builders) to
    the reference's Kronecker ordering g = (g_1 M_2 + g_2) M_3 + g_3; the dense fp64 product agrees as well."""
    cases = [(("g2_c1", "g2_c2"), "g2b1", False), (("g2_c1", "g2_c2"), "g2b3", False),
             (("g3_c1", "g3_c2", "g3_c3"), "g3", False), (("g2_c1", "g2_c2"), "lr", True)]
    for cols, p, separate in cases:
        A = operator(cols, p, separate=separate)
        for c in (1, 5):
            y = A._matmul(T(X[f"{p}_rhs{c}"])).numpy()
            assert np.allclose(y, G[f"{p}_mm{c}"], rtol=1e-4, atol=1e-5), (p, c)
        K = kron_dense64([X[c] for c in cols])
        M = K.shape[0]
        ri, rv = (X["lr_ri"], X["lr_rv"]) if separate else (X[p + "_li"], X[p + "_lv"])
        for b in range(X[p + "_li"].shape[0]):
            ref = w_dense64(X[p + "_li"][b], X[p + "_lv"][b], M) @ (K @ (w_dense64(ri[b], rv[b], M).T
                                                                          @ X[p + "_rhs5"][b].astype(np.float64)))
            assert np.abs(G[p + "_mm5"][b] - ref).max() <= 1e-4 * np.abs(ref).max(), p
