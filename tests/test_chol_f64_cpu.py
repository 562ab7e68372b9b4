"""CPU tests of the float64 exact small-N path (csrc/lo_chol_f64.hip, ABI 33): the four new C-ABI symbols, their
refusals before any launch, the sizer, and that the float32 sizer still reports what it did.  No GPU compute here."""
import ctypes
import os
import re

import torch

from linear_operator_amd import _hip
from linear_operator_amd.functions import _cholesky as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lo_cholesky_f64_workspace_bytes", "lo_cholesky_f64", "lo_tri_solve_f64", "lo_cholesky_solve_f64")
FAKE = 0x1000  # a non-null pointer that is never dereferenced: the refusals come before any launch


def test_abi_version_of_library_and_binding():
    assert _hip.ABI_VERSION >= 33
    assert _hip.load().lo_abi_version() == _hip.ABI_VERSION


def test_the_four_symbols_are_exported_declared_and_bound():
    raw = ctypes.CDLL(_hip.lib_path())
    hdr = open(os.path.join(ROOT, "include", "lo_amd.h")).read()
    declared = set(re.findall(r"\b(lo_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/lo_amd.h"
        assert name in _hip.EXPORTS and name in _hip._PROTOTYPES, f"{name} missing from _hip._PROTOTYPES"
        assert hasattr(raw, name), f"liblo_amd.so does not export {name}"
    # same argument order as the float32 calls
    for f64, f32 in (("lo_cholesky_f64_workspace_bytes", "lo_cholesky_workspace_bytes"), ("lo_cholesky_f64", "lo_cholesky_f32"),
                     ("lo_tri_solve_f64", "lo_tri_solve_f32"), ("lo_cholesky_solve_f64", "lo_cholesky_solve_f32")):
        assert _hip._PROTOTYPES[f64] == _hip._PROTOTYPES[f32]


def test_sizer():
    lib = _hip.load()
    assert lib.lo_cholesky_f64_workspace_bytes(3, 300) >= 3 * 320 * 320 * 8
    assert lib.lo_cholesky_f64_workspace_bytes(1, 1024) >= 1024 * 1024 * 8
    assert lib.lo_cholesky_f64_workspace_bytes(1, 1025) == 0
    assert lib.lo_cholesky_f64_workspace_bytes(0, 10) == 0 and lib.lo_cholesky_f64_workspace_bytes(1, 0) == 0


def test_sizes_beyond_the_kernels_are_refused_before_any_launch():
    lib = _hip.load()
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, 1, 1025, FAKE, 1 << 30, None) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_tri_solve_f64(FAKE, FAKE, FAKE, None, 1, 1025, 1, 0, 0, None) == _hip.LO_ERR_UNSUPPORTED
    assert lib.lo_cholesky_solve_f64(FAKE, FAKE, FAKE, 1, 1025, 1, 0, None) == _hip.LO_ERR_UNSUPPORTED


def test_bad_arguments_and_short_workspaces_are_refused_before_any_launch():
    lib = _hip.load()
    bad = -1  # LO_ERR_BADARG
    assert _hip._ERR[bad] == "bad argument"
    assert lib.lo_cholesky_f64(None, FAKE, FAKE, None, 1, 10, FAKE, 1 << 30, None) == bad
    assert lib.lo_cholesky_f64(FAKE, None, FAKE, None, 1, 10, FAKE, 1 << 30, None) == bad
    assert lib.lo_cholesky_f64(FAKE, FAKE, None, None, 1, 10, FAKE, 1 << 30, None) == bad
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, 1, 0, FAKE, 1 << 30, None) == bad
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, -1, 10, FAKE, 1 << 30, None) == bad
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert lib.lo_tri_solve_f64(*args, None, 1, 10, 1, 0, 0, None) == bad
        assert lib.lo_cholesky_solve_f64(*args, 1, 10, 1, 0, None) == bad
    assert lib.lo_tri_solve_f64(FAKE, FAKE, FAKE, None, 1, 10, 0, 0, 0, None) == bad
    assert lib.lo_cholesky_solve_f64(FAKE, FAKE, FAKE, 1, 0, 1, 0, None) == bad
    need = lib.lo_cholesky_f64_workspace_bytes(2, 37)
    assert need >= 2 * 64 * 64 * 8
    short = -3  # LO_ERR_WORKSPACE
    assert _hip._ERR[short] == "workspace too small"
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, 2, 37, FAKE, need - 1, None) == short
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, 2, 37, None, 0, None) == short
    # an empty batch is a success that launches nothing
    assert lib.lo_cholesky_f64(FAKE, FAKE, FAKE, None, 0, 10, None, 0, None) == 0
    assert lib.lo_tri_solve_f64(FAKE, FAKE, FAKE, None, 0, 10, 1, 0, 0, None) == 0
    assert lib.lo_cholesky_solve_f64(FAKE, FAKE, FAKE, 0, 10, 1, 0, None) == 0


def test_the_float32_sizer_reports_what_it_did_before():
    """lo_cholesky_workspace_bytes at the commit before lo_chol_f64.hip: the float32 layout is untouched."""
    lib = _hip.load()
    assert lib.lo_cholesky_workspace_bytes(3, 300) == 1236992
    assert lib.lo_cholesky_workspace_bytes(1, 1024) == 4203008


def test_routing_predicate_takes_one_dtype_and_keeps_cpu_tensors_on_aten():
    for dtype in (torch.float32, torch.float64):
        assert not FC.native_ok(torch.eye(4, dtype=dtype))
        assert not FC.native_ok(torch.eye(4, dtype=dtype), torch.ones(4, 1, dtype=dtype), solve=True)
    assert FC.SINGLE_SOLVE_MAX_N == 0 and 0 <= FC.SINGLE_SOLVE_MAX_N_F64 <= 1024
    x = FC.substitute(torch.tril(torch.ones(3, 3, dtype=torch.float64)), torch.ones(3, dtype=torch.float64))
    assert x.dtype == torch.float64 and torch.allclose(x, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
