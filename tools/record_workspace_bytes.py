"""Records what the workspace sizers of tests/workspace_cases.py report into tests/golden/workspace_bytes.json.

The recording is the upper bound of tests/test_workspace_bytes_cpu.py: a size may shrink but not grow.  It was taken
from the library of the commit before the entry points got their layout functions; run it again only on a build whose
sizes are meant to become the new bound.  No device call: the sizers are host arithmetic.

    python tools/record_workspace_bytes.py [path/to/liblo_amd.so]
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
    if len(sys.argv) > 1:  # another build's library, with the prototypes of this tree
        lib = ctypes.CDLL(sys.argv[1])
        for fn in wc.CASES:
            restype, argtypes = _hip._PROTOTYPES[fn]
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = restype, argtypes
    else:
        lib = _hip.load()
    out = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
    with open(out, "w") as f:
        json.dump(wc.sizes(lib), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
