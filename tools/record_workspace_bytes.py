"""Records what the workspace sizers of tests/workspace_cases.py report into tests/golden/workspace_bytes.json.

The recording is the upper bound of tests/test_workspace_bytes_cpu.py: a size may shrink but not grow.  It was taken
from the library of the commit before the entry points got their layout functions (the float64 rows: before their sizers
went through them); run it again only on a build whose sizes are meant to become the new bound.  No device call: the sizers are host arithmetic.

    python tools/record_workspace_bytes.py [--add] [path/to/liblo_amd.so]

--add records the rows the file does not hold yet and keeps the bound of every row it holds.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import workspace_cases as wc  # noqa: E402
from linear_operator_amd import _hip  # noqa: E402


def main():
    argv = [a for a in sys.argv[1:] if a != "--add"]
    if argv:  # another build's library, with the prototypes of this tree
        lib = ctypes.CDLL(argv[0])
        for fn in (*wc.CASES, *wc.F64_CASES):
            restype, argtypes = _hip._PROTOTYPES[fn]
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = restype, argtypes
    else:
        lib = _hip.load()
    out = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
    got = wc.sizes(lib)
    if "--add" in sys.argv[1:]:
        with open(out) as f:
            got.update(json.load(f))
    with open(out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
