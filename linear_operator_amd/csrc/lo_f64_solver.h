// lo_f64_solver.h -- host pieces the float64 solvers (lo_cg_f64.hip, lo_minres_f64.hip, lo_lanczos_f64.hip) and
// lo_matvec_f64.hip share.  A new kind of operand of the float64 solvers is added to F64Operand.
#pragma once
#include "lo_internal.h"

namespace lo {

// The operator and the preconditioner of one float64 solve as its entry point was given them: a dense matrix on
// k64_dense_mv or a callback (a closure, lo_matvec_desc_cb_f64), and a callback or no preconditioner.  Vectors [B, N, c].
struct F64Operand {
  const double* A;     // [B, N, N] or nullptr: `matvec` is the operator
  const double* diag;  // [B, N] added to A, or nullptr
  lo_matvec_cb_f64 matvec;
  void* matvec_user;
  lo_matvec_cb_f64 precond_cb;  // nullptr: no preconditioner
  void* precond_user;
  int64_t B, N, c;
  void* stream;

  bool valid() const { return A || matvec; }
  // y = A v; a callback's non-zero return is LO_ERR_LAUNCH
  int op(const double* v, double* y) const {
    if (A) return f64_dense_mv(A, diag, v, y, B, N, c, (hipStream_t)stream);
    return matvec(matvec_user, v, y, B, N, c, stream) ? LO_ERR_LAUNCH : LO_OK;
  }
  // y = P^-1 v (no preconditioner: y = v)
  int pre(const double* v, double* y) const {
    if (precond_cb) return precond_cb(precond_user, v, y, B, N, c, stream) ? LO_ERR_LAUNCH : LO_OK;
    return f64_copy(v, y, (size_t)B * N * c, (hipStream_t)stream);
  }
};

// a control block (or n flag words) from the workspace to the host, complete when the call returns
template <typename T>
int f64_read_back(T* host, const T* dev, hipStream_t st, size_t n = 1) {
  LO_HIP_CHECK(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  LO_HIP_CHECK(hipStreamSynchronize(st));
  return LO_OK;
}

// grid of a launch with one thread of a kThreads block per element
inline dim3 elem_grid(size_t total) { return dim3((unsigned)((total + kThreads - 1) / kThreads)); }

}  // namespace lo
