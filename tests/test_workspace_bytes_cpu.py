"""Workspace sizes of the entry points beside the solvers, on the CPU (the sizers make no HIP call): every row of
tests/workspace_cases.py.  Each entry point is sized by the layout function that carves its workspace, so a size is what
the entry point takes: it covers the buffers the entry point provably uses, and it may not exceed what the hand-kept
formulas reported before (tests/golden/workspace_bytes.json, recorded by tools/record_workspace_bytes.py from the commit
before the layout functions).  lo_precond_apply_workspace_bytes shrinks where the rank needs no padding: it used to count
a padded copy of Q that the apply never takes."""
import json
import os

import pytest

import workspace_cases as wc
from linear_operator_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "workspace_bytes.json")) as f:
    RECORDED = json.load(f)
ROWS = [(fn, args, needed) for fn, rows in wc.CASES.items() for args, needed in rows]
ROWS += [(fn, args, needed) for fn, rows in wc.F64_CASES.items() for args, needed in rows]


def test_the_recording_covers_the_table():
    assert sorted(RECORDED) == sorted(wc.key(fn, args) for fn, args, _ in ROWS)
    assert len(wc.CASES) == 11 and all(len(rows) >= 2 for rows in wc.CASES.values())
    assert len(wc.F64_CASES) == 4 and all(len(rows) >= 3 for rows in wc.F64_CASES.values())


@pytest.mark.parametrize("fn,args,needed", ROWS, ids=[wc.key(fn, args) for fn, args, _ in ROWS])
def test_sizes_within_the_recorded_ones_and_above_the_needed_buffers(fn, args, needed):
    got, was = int(getattr(_hip.load(), fn)(*args)), RECORDED[wc.key(fn, args)]
    print(fn, args, got, "recorded", was, "needed", needed)
    assert needed <= got <= was
    if needed == 0:  # a refused shape stays refused
        assert got == 0


def test_the_apply_counts_the_padded_copy_only_where_it_is_taken():
    lib = _hip.load()
    for B, N, c in wc.APPLY_SHAPES:
        for k in wc.APPLY_RANKS:
            got = int(lib.lo_precond_apply_workspace_bytes(B, N, k, c))
            copy = 4 * B * N * wc.padded_rank(k)
            was = RECORDED[wc.key("lo_precond_apply_workspace_bytes", (B, N, k, c))]
            if k == wc.padded_rank(k):
                assert got <= was - copy
            else:
                assert got >= copy
