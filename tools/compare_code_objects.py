#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds: tools/compare_code_objects.py PARENT_DIR NEW_DIR

Each directory holds the device assembly files (*gfx950*.s) that `hipcc <Makefile flags> --save-temps -c` leaves
behind, one per translation unit.  For every kernel: the resource metadata of both builds and whether the instruction
streams are identical (comments, debug labels and blank lines ignored).  Prints one line per kernel."""
import glob
import os
import re
import sys

KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        ins = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith((".loc", ".file", ".cfi", ".Ltmp", ".p2align")):
                ins.append(ln)
        out[name] = {"ins": ins}
    # metadata: the YAML note at the end of the file, one block per kernel
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        nm = re.search(r"\.name:\s+(\w+)", blk)
        if not nm or nm.group(1) not in out:
            continue
        for k in KEYS:
            v = re.search(re.escape(k) + r":\s+(\d+)", blk)
            out[nm.group(1)][k] = int(v.group(1)) if v else -1
    return {k: v for k, v in out.items() if ".vgpr_count" in v}


def main():
    parent, new = sys.argv[1], sys.argv[2]
    print("# kernel | vgpr sgpr lds scratch spills (parent -> new) | instructions (parent -> new) | flag")
    ndiff = 0
    for f in sorted(glob.glob(os.path.join(new, "*gfx950*.s"))):
        kp, kn = kernels(os.path.join(parent, os.path.basename(f))), kernels(f)
        tu = os.path.basename(f).split("-hip-")[0]
        for name in sorted(set(kp) | set(kn)):
            a, b = kp.get(name), kn.get(name)
            if a is None or b is None:
                print(f"{tu} {name} | only in {'new' if a is None else 'parent'}")
                ndiff += 1
                continue
            same = a["ins"] == b["ins"]
            ndiff += not same
            meta = " ".join(f"{a[k]}->{b[k]}" if a[k] != b[k] else str(a[k]) for k in KEYS)
            print(f"{tu} {name} | {meta} | {len(a['ins'])}->{len(b['ins'])} | {'ISA identical' if same else 'differs'}")
    print(f"# {ndiff} kernel(s) differ")


if __name__ == "__main__":
    main()
