#!/usr/bin/env python3
"""The five gates of KernelLinearOperator against an earlier commit's, string for string, on the CPU.

    python tools/compare_kernel_gates.py [REV]        (REV defaults to HEAD)

Loads REV's operators/kernel_linear_operator.py from `git show` under another module name next to the working tree's,
builds the same operators with both classes over the grid below and compares `_native_refusal`, `_native_f64_refusal`,
`_native_grad_refusal`, `_native_task_refusal` and `_native_param_refusal` with check_device True and False (an
exception counts as its type and text).  Where the working tree has `_native_variant`, it is also held to the gates:
the variant returned is the one whose gate passes, None when none does, and no operator passes two.  Needs neither the
library nor a GPU.  Prints the counts and exits 1 on any difference."""
import importlib.util
import itertools
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd.operators import kernel_linear_operator as new_mod  # noqa: E402

PATH = "linear_operator_amd/operators/kernel_linear_operator.py"
GATES = ("_native_refusal", "_native_f64_refusal", "_native_grad_refusal", "_native_task_refusal", "_native_param_refusal")
TAG_OF_GATE = {"_native_refusal": (None, torch.float32), "_native_f64_refusal": (None, torch.float64),
               "_native_grad_refusal": ("grad", torch.float32), "_native_task_refusal": ("task", torch.float32),
               "_native_param_refusal": ("param", torch.float32)}


def load_parent(rev):
    src = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{PATH}"], check=True, capture_output=True, text=True).stdout
    name = "linear_operator_amd.operators._kernel_linear_operator_parent"
    spec = importlib.util.spec_from_loader(name, loader=None, origin=f"{rev}:{PATH}")
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "linear_operator_amd.operators"
    sys.modules[name] = mod
    exec(compile(src, f"{rev}:{PATH}", "exec"), mod.__dict__)
    return mod


def untagged(x1, x2, lengthscale, outputscale):
    return covariance.rbf(x1, x2, lengthscale, outputscale)


def rq_code_without_tag(x1, x2, lengthscale, outputscale):
    return covariance.rbf(x1, x2, lengthscale, outputscale)


rq_code_without_tag.native_family = _hip.LO_KERNEL_RQ

FUNCS = [*covariance.FAMILIES.values(), *covariance.GRAD_FAMILIES.values(), *covariance.TASK_FAMILIES.values(),
         *covariance.PARAM_FAMILIES.values(), untagged, rq_code_without_tag]
PARAM_SETS = ("ls_os", "task", "alpha", "period", "ls")
TWISTS = ("none", "nonbatch_ls", "nonbatch_os", "nonbatch_extra", "nontensor", "float_lengthscale", "x2_width",
          "mixed_ls", "mixed_extra", "rectangular")


def build_args(func, DX, dtype, outs, pset, batch, width, T, twist):
    """(x1, x2, kwargs) of one operator; None where the twist does not apply."""
    g = torch.Generator().manual_seed(0)
    other = torch.float64 if dtype == torch.float32 else torch.float32
    x1 = torch.rand(*batch, 5, DX, generator=g).to(dtype)
    x2 = x1
    if twist == "x2_width":
        x2 = torch.rand(*batch, 5, DX + 1, generator=g).to(dtype)
    elif twist == "rectangular":
        x2 = torch.rand(*batch, 7, DX, generator=g).to(dtype)
    w = {"one": 1, "ard": DX, "coords": max(DX - 1, 1), "wrong": DX + 1}[width]
    params = {"lengthscale": torch.ones(*batch, 1, w, dtype=other if twist == "mixed_ls" else dtype)}
    nonbatch = {"outputscale": 0, "alpha": 0}
    if pset != "ls":
        params["outputscale"] = torch.ones(batch, dtype=dtype)
    extra = {"task": "task_covar", "alpha": "alpha", "period": "period_length"}.get(pset)
    edtype = other if twist == "mixed_extra" else dtype
    if pset == "task":
        params["task_covar"] = torch.eye(T, dtype=edtype).expand(*batch, T, T).contiguous()
    elif pset == "alpha":
        params["alpha"] = torch.ones(batch, dtype=edtype)
    elif pset == "period":
        params["period_length"] = torch.ones(*batch, 1, w, dtype=edtype)
    if twist in ("mixed_extra", "nonbatch_extra") and extra is None:
        return None
    if twist == "nonbatch_ls":
        nonbatch["lengthscale"] = 1
    elif twist == "nonbatch_os":
        del nonbatch["outputscale"]
    elif twist == "nonbatch_extra":
        nonbatch[extra] = 1 if pset != "alpha" else 2
    elif twist == "nontensor":
        params["flag"] = True
    elif twist == "float_lengthscale":
        params["lengthscale"] = 1.0
    kwargs = dict(covar_func=func, num_outputs_per_input=(1, 1) if outs == "one" else (DX + 1, DX + 1),
                  num_nonbatch_dimensions=nonbatch, **params)
    return x1, x2, kwargs


def ask(op, gate, check_device):
    try:
        return getattr(op, gate)(check_device=check_device)
    except Exception as e:  # noqa: BLE001 (an exception is part of what the gate answers)
        return f"raised {type(e).__name__}: {e}"


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    old_mod = load_parent(rev)
    operators = comparisons = differ = resolved = wrong = 0
    passes = {g: 0 for g in GATES}
    grid = itertools.product(FUNCS, (1, 2, 3, 17, 33), (torch.float32, torch.float64), ("one", "grad"), PARAM_SETS,
                             ((), (2,)), ("one", "ard", "coords", "wrong"), TWISTS)
    for func, DX, dtype, outs, pset, batch, width, twist in grid:
        for T in ((1, 8, 9) if pset == "task" else (0,)):
            args = build_args(func, DX, dtype, outs, pset, batch, width, T, twist)
            if args is None:
                continue
            x1, x2, kwargs = args
            built = []
            for mod in (old_mod, new_mod):
                try:
                    built.append(mod.KernelLinearOperator(x1, x2, **kwargs))
                except Exception as e:  # noqa: BLE001
                    built.append(f"raised {type(e).__name__}: {e}")
            operators += 1
            if isinstance(built[0], str) or isinstance(built[1], str):
                comparisons += 1
                differ += built[0] != built[1]
                continue
            passing = []
            for gate, check_device in itertools.product(GATES, (True, False)):
                a, b = ask(built[0], gate, check_device), ask(built[1], gate, check_device)
                comparisons += 1
                if a != b:
                    differ += 1
                    print(f"DIFFERS {func.__name__} DX={DX} {dtype} {outs} {pset} {batch} {width} T={T} {twist} "
                          f"{gate}({check_device}): {a!r} != {b!r}")
                if not check_device and a is None:
                    passing.append(gate)
                    passes[gate] += 1
            if hasattr(built[1], "_native_variant"):
                v = built[1]._native_variant(check_device=False)
                got = None if v is None else (v.tag, v.dtype)
                want = TAG_OF_GATE[passing[0]] if len(passing) == 1 else None
                resolved += 1
                if len(passing) > 1 or got != want:
                    wrong += 1
                    print(f"RESOLVER {func.__name__} DX={DX} {dtype} {outs} {pset} {batch} {width} T={T} {twist}: "
                          f"gates passing {passing}, _native_variant {got}")
    print(f"parent {rev}: {operators} operators, {comparisons} comparisons, {differ} differ")
    print("operators passing each gate with check_device=False: " + ", ".join(f"{g} {n}" for g, n in passes.items()))
    print(f"_native_variant(check_device=False) against the gates: {resolved} operators, {wrong} wrong or passing two")
    return 1 if differ or wrong else 0


if __name__ == "__main__":
    sys.exit(main())
