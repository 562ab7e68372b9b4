// _lo_pyfast: the native entry of the headline solve's session step.  A CPython extension against the plain
// C API -- no libtorch, no HIP, and NOT linked against liblo_amd.so: Python hands it the address of the entry point out of
// the CDLL that _hip.load() holds (bind), so it calls the very image ctypes loaded.  One hot function, session_solve: what
// ctypes spent on two byref structs, six argument conversions and eight field reads per solve is a stack frame here.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include "../../include/lo_amd.h"

namespace {

using session_solve_fn = int (*)(struct lo_cg_session*, const float*, float*, lo_cg_info*, lo_cg_plan*, void*);
session_solve_fn g_session_solve = nullptr;

// An address from a Python int (0 .. 2^64 - 1); anything else: TypeError / OverflowError set, false.
bool address(PyObject* o, void** out) {
  if (!PyLong_Check(o)) {
    PyErr_Format(PyExc_TypeError, "an address is an int, not %.80s", Py_TYPE(o)->tp_name);
    return false;
  }
  *out = PyLong_AsVoidPtr(o);
  return !(*out == nullptr && PyErr_Occurred());
}

// bind(lo_cg_session_solve_f32: int) -> None.  0 unbinds.
PyObject* bind(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 1) {
    PyErr_Format(PyExc_TypeError, "bind() takes 1 argument (%zd given)", nargs);
    return nullptr;
  }
  void* p = nullptr;
  if (!address(args[0], &p)) return nullptr;
  g_session_solve = reinterpret_cast<session_solve_fn>(p);
  Py_RETURN_NONE;
}

PyObject* bound(PyObject*, PyObject*) { return PyBool_FromLong(g_session_solve != nullptr); }

// session_solve(handle, rhs, x, stream) -> (rc, iterations, matvecs, tolerance_reached, nan_detected, skipped,
// mean_residual, plan.rspace): lo_cg_session_solve_f32 with its result structs on this frame.  rc is returned as it is
// (LO_ERR_UNSUPPORTED is a decision of the library); the other fields are meaningful when rc == 0.  The GIL is released
// around the call: the host spins on the ticket of the launch there.
PyObject* session_solve(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 4) {
    PyErr_Format(PyExc_TypeError, "session_solve() takes 4 arguments (%zd given)", nargs);
    return nullptr;
  }
  const session_solve_fn fn = g_session_solve;
  if (!fn) {
    PyErr_SetString(PyExc_RuntimeError, "_lo_pyfast is not bound to liblo_amd.so (bind() first)");
    return nullptr;
  }
  void *handle, *rhs, *x, *stream;
  if (!address(args[0], &handle) || !address(args[1], &rhs) || !address(args[2], &x) || !address(args[3], &stream))
    return nullptr;
  lo_cg_info info = {};
  lo_cg_plan plan = {};
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = fn(static_cast<struct lo_cg_session*>(handle), static_cast<const float*>(rhs), static_cast<float*>(x), &info, &plan,
          stream);
  Py_END_ALLOW_THREADS
  PyObject* out = PyTuple_New(8);
  if (!out) return nullptr;
  PyObject* items[8] = {PyLong_FromLong(rc),
                        PyLong_FromLong(info.iterations),
                        PyLong_FromLong(info.matvecs),
                        PyBool_FromLong(info.tolerance_reached),
                        PyBool_FromLong(info.nan_detected),
                        PyBool_FromLong(info.skipped),
                        PyFloat_FromDouble(info.mean_residual),
                        PyLong_FromLong(plan.rspace)};
  bool ok = true;
  for (int i = 0; i < 8; ++i) ok = ok && items[i];
  if (!ok) {
    for (int i = 0; i < 8; ++i) Py_XDECREF(items[i]);
    Py_DECREF(out);
    return nullptr;
  }
  for (int i = 0; i < 8; ++i) PyTuple_SET_ITEM(out, i, items[i]);
  return out;
}

PyMethodDef methods[] = {
    {"bind", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(bind)), METH_FASTCALL,
     "bind(address of lo_cg_session_solve_f32 in the loaded liblo_amd.so); 0 unbinds"},
    {"bound", bound, METH_NOARGS, "True once bind() has been given an address"},
    {"session_solve", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(session_solve)), METH_FASTCALL,
     "session_solve(handle, rhs, x, stream) -> (rc, iterations, matvecs, tolerance_reached, nan_detected, skipped, "
     "mean_residual, plan.rspace)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module = {PyModuleDef_HEAD_INIT, "_lo_pyfast", "native entry of the session solve (see csrc/lo_pyfast.cpp)", -1,
                      methods,               nullptr,      nullptr,                                                    nullptr,
                      nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__lo_pyfast(void) { return PyModule_Create(&module); }
