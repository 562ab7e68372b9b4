"""The native entry of the session solve (csrc/lo_pyfast.cpp -> lib/_lo_pyfast.so) without a GPU: the Makefile
rule and its skip, the module's argument handling, the values it hands back (bound to a host stand-in of
lo_cg_session_solve_f32 with the library's own struct types), and the optional loader with the setter in kernels."""
import ctypes as C
import os
import subprocess

import pytest

from linear_operator_amd import _hip
from linear_operator_amd import kernels as K

CSRC = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), "csrc")
SOLVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_hip.CgInfo), C.POINTER(_hip.CgPlan),
                       C.c_void_p)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """The module as the csrc Makefile builds it, in a directory of its own, imported by the loader's own code."""
    path = str(tmp_path_factory.mktemp("pyfast") / "_lo_pyfast.so")
    r = subprocess.run(["make", "-C", CSRC, f"PYFAST={path}", path], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(path), (r.stdout[-2000:], r.stderr[-2000:])
    old = _hip._FAST_PATH
    _hip._FAST_PATH = path
    try:
        mod = _hip._import_fast()
    finally:
        _hip._FAST_PATH = old
    yield mod
    mod.bind(0)


@pytest.fixture
def fresh_loader():
    """_hip.fast() and the setter of kernels asked anew inside the test, and again after it."""
    def reset():
        _hip._fast = False
        K._fast_module = K._UNSET
        K._fast_mode = None

    reset()
    yield
    reset()


def test_builds_and_imports(built):
    assert built.__name__ == "_lo_pyfast"
    assert callable(built.session_solve) and callable(built.bind) and built.bound() is False


def test_the_tree_s_build_is_what_the_loader_returns(fresh_loader):
    # build() ran the same Makefile: the module beside liblo_amd.so loads, is bound, and is in force by default
    mod = _hip.fast()
    assert mod is not None and mod.bound() is True and _hip.fast() is mod
    assert K.cg_fast_entry(None) == "native"
    assert K.cg_fast_entry(False) == "ctypes"
    assert K.cg_fast_entry(True) == "native"
    assert K.cg_fast_entry() == "native"
    with pytest.raises(TypeError):
        K.cg_fast_entry(1)


def test_unbound_use_and_wrong_arguments_raise(built):
    built.bind(0)
    with pytest.raises(RuntimeError, match="not bound"):
        built.session_solve(1, 2, 3, 4)
    for args in ((), (1,), (1, 2, 3), (1, 2, 3, 4, 5)):
        with pytest.raises(TypeError):
            built.session_solve(*args)
    with pytest.raises(TypeError):
        built.bind()
    with pytest.raises(TypeError):
        built.bind(1, 2)
    with pytest.raises(TypeError):
        built.bind("0x10")
    with pytest.raises(TypeError):
        built.session_solve(x=1)


def test_values_through_a_host_stand_in(built):
    seen = []

    def stand_in(handle, rhs, x, info, plan, stream):
        seen.append((handle, rhs, x, stream))
        if handle == 7:
            return _hip.LO_ERR_UNSUPPORTED
        i, p = info.contents, plan.contents
        i.iterations, i.matvecs, i.tolerance_reached, i.nan_detected, i.skipped = 11, 12, 1, 0, 0
        i.mean_residual, p.rspace = 0.1, 2
        return 0

    cb = SOLVE_FN(stand_in)
    built.bind(C.cast(cb, C.c_void_p).value)
    assert built.bound() is True
    out = built.session_solve(2**63 + 5, 16, 32, 0)
    assert seen == [(2**63 + 5, 16, 32, None)]  # (a null stream reaches a ctypes callback as None)
    assert out == (0, 11, 12, True, False, False, float(C.c_float(0.1).value), 2)
    assert [type(v) for v in out] == [int, int, int, bool, bool, bool, float, int]
    rc = built.session_solve(7, 16, 32, 99)[0]
    assert rc == _hip.LO_ERR_UNSUPPORTED and seen[-1] == (7, 16, 32, 99)
    for bad in ((1.0, 2, 3, 4), (1, None, 3, 4), (1, 2, "3", 4), (1, 2, 3, 2**64)):
        with pytest.raises((TypeError, OverflowError)):
            built.session_solve(*bad)
    assert len(seen) == 2  # (nothing was called with a bad argument)


def test_import_masked_the_ctypes_path_is_in_force(fresh_loader, monkeypatch):
    def refuse():
        raise ImportError("masked")

    monkeypatch.setattr(_hip, "_import_fast", refuse)
    assert _hip.fast() is None
    assert K.cg_fast_entry(None) == "ctypes"
    assert K.cg_fast_entry(False) == "ctypes"
    with pytest.raises(_hip.HipExtensionError, match="not available"):
        K.cg_fast_entry(True)
    assert K.cg_fast_entry(None) == "ctypes"


def test_file_missing_the_ctypes_path_is_in_force(fresh_loader, monkeypatch, tmp_path):
    monkeypatch.setattr(_hip, "_FAST_PATH", str(tmp_path / "_lo_pyfast.so"))
    assert _hip.fast() is None and K.cg_fast_entry(None) == "ctypes"


def test_makefile_dry_run_without_python_headers_skips_the_target():
    r = subprocess.run(["make", "-n", "-C", CSRC, "PYINC="], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "lo_pyfast.cpp -o" not in r.stdout and "lo_pyfast: no Python.h" in r.stdout, r.stdout[-2000:]
    r = subprocess.run(["make", "-n", "-C", CSRC, "-W", "lo_pyfast.cpp"], capture_output=True, text=True)
    assert r.returncode == 0 and "lo_pyfast.cpp -o" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
