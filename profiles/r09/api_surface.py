"""Dump the public surface of linear_operator_amd.kernels and ._hip: name, signature / value."""
import ctypes
import inspect
import sys

sys.path.insert(0, sys.argv[1])
from linear_operator_amd import _hip, kernels  # noqa: E402

EXTRA = {"kernels": ["_eigform_due", "_cg_params", "_with_diag", "_native_lanczos_layout"], "_hip": []}


def describe(obj):
    if isinstance(obj, type) and issubclass(obj, ctypes.Structure):
        return "struct " + repr([(n, t.__name__) for n, t in obj._fields_])
    if isinstance(obj, type) and issubclass(obj, ctypes._CFuncPtr):
        return "cfunctype " + repr((getattr(obj._restype_, "__name__", None), [a.__name__ for a in obj._argtypes_]))
    if isinstance(obj, type):
        members = sorted((n, str(inspect.signature(m))) for n, m in vars(obj).items()
                         if callable(m) and (not n.startswith("_") or n == "__init__"))
        try:
            sig = str(inspect.signature(obj))
        except (TypeError, ValueError):
            sig = "?"
        return f"class {sig} bases={[b.__name__ for b in obj.__bases__]} {members}"
    if callable(obj):
        return "def " + str(inspect.signature(obj))
    if isinstance(obj, (int, float, str, bool, type(None), dict, tuple)):
        return "const " + repr(obj)
    if isinstance(obj, list):
        return "const " + repr(sorted(obj) if all(isinstance(x, str) for x in obj) else obj)
    return None


for mod in (kernels, _hip):
    short = mod.__name__.rsplit(".", 1)[-1]
    for name in sorted(vars(mod)):
        obj = vars(mod)[name]
        if inspect.ismodule(obj) or (name.startswith("_") and name not in EXTRA[short]):
            continue
        if getattr(obj, "__module__", mod.__name__) not in (mod.__name__, "ctypes") and not isinstance(obj, (int, float, str, dict, list, tuple, type(None))):
            continue  # imported helpers (dataclass, Optional, ...)
        d = describe(obj)
        if d is not None:
            print(f"{short}.{name}: {d}")
