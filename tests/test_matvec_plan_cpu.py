"""The matvec plan layer's workspace sizes on the CPU (the sizing entry points make no HIP call): every descriptor of
tests/matvec_plan_cases.py, at one and three columns, through lo_matvec_workspace_bytes and the three solver sizing
functions.  Since the plan of a kind is sized by the function that builds it, a size is what the build takes: it may not
exceed what the hand-kept sizing copies reported before (tests/golden/matvec_plan_bytes.json, recorded from the commit
before the plan functions were merged), and it covers the buffers the kind provably needs."""
import ctypes
import json
import os

import pytest

import matvec_plan_cases as mc
from linear_operator_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "matvec_plan_bytes.json")) as f:
    RECORDED = json.load(f)
SIZERS = ("lo_matvec_workspace_bytes", "lo_cg_workspace_bytes", "lo_minres_workspace_bytes",
          "lo_lanczos_workspace_bytes")


def test_the_recording_covers_the_table():
    assert sorted(RECORDED) == sorted(f"{name}/c{c}" for name in mc.CASES for c in mc.COLS)
    assert all(sorted(v) == sorted(SIZERS) for v in RECORDED.values())


@pytest.mark.parametrize("c", mc.COLS)
@pytest.mark.parametrize("name", mc.CASES)
def test_sizes_within_the_recorded_ones_and_above_the_needed_buffers(name, c):
    lib = _hip.load()
    case = mc.build(name)
    got, was, need = mc.sizes(lib, case.desc, c), RECORDED[f"{name}/c{c}"], case.need(c)
    print(name, c, got, "recorded", was, "needed", need)
    for fn in SIZERS:
        assert need <= got[fn] <= was[fn], (fn, need, got[fn], was[fn])
    # (the solvers lay the plan out behind their own vectors: at least x, r, p, Ap / three Lanczos-sized blocks)
    nv = 4 * case.desc.B * case.desc.N * c
    assert got["lo_cg_workspace_bytes"] >= need + 4 * nv
    assert got["lo_minres_workspace_bytes"] >= need + 3 * nv
    assert got["lo_lanczos_workspace_bytes"] >= need + nv


def _invalid():
    """One refused descriptor per kind: the sizing pass stops at the refusal and must neither crash nor keep anything."""
    out = []
    for name, edit in (("lowrank_r5", lambda s: setattr(s, "R", 0)), ("dense_plain", lambda s: setattr(s, "A0", None)),
                       ("kron_3x5", lambda s: setattr(s, "n2", 4)), ("toeplitz_33", lambda s: setattr(s, "R", 32)),
                       ("ski", lambda s: setattr(s, "A0", None)), ("ski_grid_2d", lambda s: setattr(s, "R", 34)),
                       ("hadamard", lambda s: setattr(s, "n2", 0)), ("masked_dense", lambda s: setattr(s, "N", 5)),
                       ("sum3", lambda s: setattr(s, "nterms", 1))):
        case = mc.build(name)
        s = case.desc.c_struct()
        edit(s)
        out.append((name, case, s))
    return out


def test_refused_descriptors_are_sized_without_their_buffers():
    lib = _hip.load()
    for name, case, s in _invalid():
        got = int(lib.lo_matvec_workspace_bytes(ctypes.byref(s), 3))
        assert got <= 256, (name, got)  # (refused before the first buffer is taken: only the fixed tail)
        cg, mr = mc.cg_params(3), mc.minres_params(3)
        assert lib.lo_cg_workspace_bytes(ctypes.byref(s), None, ctypes.byref(cg)) > 0
        assert lib.lo_minres_workspace_bytes(ctypes.byref(s), None, ctypes.byref(mr)) > 0
        assert lib.lo_lanczos_workspace_bytes(ctypes.byref(s), 3, mc.LANCZOS_ITERS) > 0


def test_the_csr_sizes_share_one_layout():
    lib = _hip.load()
    B, N, J, M = 2, 50, 4, 20
    need = 2 * 4 * B * (M + 1) + 2 * 4 * B * N * J
    a, b = lib.lo_interp_t_workspace_bytes(B, N, J, M), lib.lo_interp_plan_bytes(B, N, J, M)
    assert a == b and need <= a <= need + 4 * 256 + 256  # (four buffers, each aligned to 256 bytes, and the tail)
