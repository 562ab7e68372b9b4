#!/usr/bin/env python3
"""Masked-operator microbenchmark: per-product time of the native LO_OP_MASKED product (csrc/lo_masked.hip) against the
ATen composition on the same GPU, on device events after warm-up.

  native        K.matvec on the masked descriptor
  composition   zeros -> index_copy through the kept index list -> K.matvec of the base -> index_select: the operator's
                fallback, free of host synchronisation.  This is what the native product has to beat.
  reference     the reference's own form, `res[..., mask, :] = rhs` and `res[..., mask, :]` with the boolean mask: each
                indexing runs a nonzero and waits for its count.  For the record only.
  base          the base's product alone on the unmasked size (what the masked product is priced against)

The three are timed alternately in `--rounds` rounds; the table gives the median and the spread (min .. max) of each.
Shapes: dense N0 4096 / 16384 at mask fractions 0.5 / 0.9, Kronecker 256 (x) 64 and 256 (x) 256 at 0.7, and the masked
low-rank 8192 x 32 (its gathered form against the composition around the full root); c = 1, 17.
Usage:  python tools/mb_masked.py [--reps 20] [--rounds 5] [--shapes a,b] [--cols 1,17]   One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_operator_amd import kernels as K  # noqa: E402

SHAPES = {
    "dense4096_f50": dict(kind="dense", n=4096, frac=0.5),
    "dense4096_f90": dict(kind="dense", n=4096, frac=0.9),
    "dense16384_f50": dict(kind="dense", n=16384, frac=0.5),
    "dense16384_f90": dict(kind="dense", n=16384, frac=0.9),
    "kron256x64_f70": dict(kind="kron", n1=256, n2=64, frac=0.7),
    "kron256x256_f70": dict(kind="kron", n1=256, n2=256, frac=0.7),
    "lowrank8192x32_f70": dict(kind="lowrank", n=8192, R=32, frac=0.7),
}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--cols", default="1,17")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    for name in args.shapes.split(","):
        s = SHAPES[name]
        if s["kind"] == "dense":
            n0 = s["n"]
            base = K.dense_diag_descriptor(rn(1, n0, n0) / n0 ** 0.5, torch.rand(1, n0, device="cuda", generator=g))
        elif s["kind"] == "kron":
            n0 = s["n1"] * s["n2"]
            base = K.kron_diag_descriptor(rn(1, s["n1"], s["n1"]) / s["n1"] ** 0.5, rn(1, s["n2"], s["n2"]) / s["n2"] ** 0.5,
                                          torch.full((1,), 0.3, device="cuda"), const_diag=True)
        else:
            n0 = s["n"]
            Croot, dfull = rn(1, n0, s["R"]) / s["R"] ** 0.5, torch.rand(1, n0, device="cuda", generator=g)
            base = K.lowrank_diag_descriptor(Croot, dfull)
        mask = torch.rand(n0, device="cuda", generator=g) < s["frac"]
        idx = torch.nonzero(mask).squeeze(-1)
        M = idx.numel()
        if s["kind"] == "lowrank":  # the operator's lowering: the gathered root, an ordinary low-rank descriptor
            native = K.lowrank_diag_descriptor(Croot.index_select(1, idx), dfull.index_select(1, idx))
        else:
            native = K.masked_descriptor(base, idx)
        for c in (int(k) for k in args.cols.split(",")):
            v = rn(1, M, c)
            vfull = rn(1, n0, c)

            def composition():
                u = torch.zeros(1, n0, c, device="cuda").index_copy_(-2, idx, v)
                return K.matvec(base, u).index_select(-2, idx)

            def reference():
                u = torch.zeros(1, n0, c, device="cuda")
                u[..., mask, :] = v
                return K.matvec(base, u)[..., mask, :]

            fns = dict(native=lambda: K.matvec(native, v), composition=composition, reference=reference,
                       base=lambda: K.matvec(base, vfull))
            yr = composition()
            err = float((fns["native"]() - yr).abs().max() / yr.abs().max())
            for _ in range(3):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            t = {k: [] for k in fns}
            for _ in range(args.rounds):  # alternate: all see the same state of the machine
                for k, fn in fns.items():
                    t[k].append(timed(fn, args.reps))
            med = {k: statistics.median(x) for k, x in t.items()}
            out = dict(shape=name, n0=n0, M=M, c=c, max_rel_diff=err)
            for k in fns:
                out[k + "_us"] = round(med[k], 1)
                out[k + "_spread"] = [round(min(t[k]), 1), round(max(t[k]), 1)]
            out["speedup"] = round(med["composition"] / med["native"], 2)
            out["faster_beyond_spread"] = bool(max(t["native"]) < min(t["composition"]))
            out["native_over_base"] = round(med["native"] / med["base"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
