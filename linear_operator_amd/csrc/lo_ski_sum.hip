// lo_ski_sum.hip -- additive structured kernel interpolation: K ~= sum_{p < P} W_l,p T_p W_r,p^T, one 1-D grid of M
// points per term (input dimension) over the same N rows.
//   SumBatchLinearOperator._matmul  (sum_batch_linear_operator.py, block_linear_operator.py:104-118) over
//   InterpolatedLinearOperator._matmul (interpolated_linear_operator.py:192-219) of a Toeplitz base
// The P terms of a member are P more grid members to the kernels of lo_ski.hip: member g = b * P + p of the interpolation
// arrays [B, P, N, J] and of the columns [B, P, M].  One product:
//   u_p = W_r,p^T v   k_interp_t_* over the G = B P members, member g reading v[g / P] (no [P, N, c] copy of v)
//   T_p u_p           k_tz_mv / k_tz_reduce over the G members
//   k_interp_sum      y[b, n, s] = sum_p (sum_j lv[b, p, n, j] (T_p u_p)[idx[b, p, n, j], s]) + d o v: a thread per output
//                     element, p ascending outside and j ascending inside, the diagonal term last as in k_interp -- no
//                     float atomics, no [P, N, c] intermediate.  With P == 1 the operations are those of k_interp.
// Index entries outside [0, M) contribute nothing: no kernel reads outside the arrays it was given.
#include <algorithm>
#include <climits>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

constexpr int64_t kSkiSumMaxMembers = 65535;  // grid members B * P: the z extent of the Toeplitz launch

__global__ __launch_bounds__(kThreads) void k_interp_sum(const int64_t* __restrict__ idx, const float* __restrict__ vals,
                                                          int64_t B, int P, int64_t N, int J, int64_t M,
                                                          const float* __restrict__ u, int c,
                                                          const float* __restrict__ dd, int dd_mode,
                                                          const float* __restrict__ v, float* __restrict__ y,
                                                          const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t total = (size_t)B * N * c;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t row = e / c;  // b * N + n
    const int col = (int)(e % c);
    const size_t b = row / N;
    const size_t n = row - b * N;
    float sum = 0.f;
    for (int p = 0; p < P; ++p) {
      const size_t g = b * P + p;
      const int64_t* ir = idx + (g * N + n) * J;
      const float* wr = vals + (g * N + n) * J;
      const float* ug = u + g * M * c + col;
      float acc = 0.f;
      for (int j = 0; j < J; ++j) {
        const int64_t m = ir[j];
        const float t = (m >= 0 && m < M) ? ug[m * c] : 0.f;
        acc = fmaf(t, wr[j], acc);
      }
      sum = p == 0 ? acc : sum + acc;
    }
    if (dd_mode == LO_DIAG_FULL) sum = fmaf(dd[row], v[e], sum);
    else if (dd_mode == LO_DIAG_CONST) sum = fmaf(dd[b], v[e], sum);
    y[e] = sum;
  }
}

static bool ski_sum_shape_ok(int64_t B, int64_t P, int64_t N, int64_t J, int64_t M) {
  return B >= 1 && P >= 1 && P <= LO_SKI_SUM_MAX_TERMS && B <= kSkiSumMaxMembers / P && interp_shape_ok(B * P, N, J, M);
}

static int interp_sum(const int64_t* idx, const float* vals, int64_t B, int64_t P, int64_t N, int64_t J, int64_t M,
                      const float* u, int64_t c, const float* dd, int dd_mode, const float* v, float* y, const int* stop,
                      hipStream_t st) {
  const size_t total = (size_t)B * N * c;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((total + kThreads - 1) / kThreads, 8192));
  LO_PROF_BEGIN("ski_interp_sum", st);
  hipLaunchKernelGGL(k_interp_sum, dim3(grid), dim3(kThreads), 0, st, idx, vals, B, (int)P, N, (int)J, M, u, (int)c, dd,
                     dd_mode, v, y, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int ski_sum_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !interp_ptrs_ok(op->interp)) return LO_ERR_BADARG;
  if (op->nterms < 1 || op->n2 < 1 || op->R < 1 || op->B < 1 || op->N < 1) return LO_ERR_BADARG;
  if (op->nterms > LO_SKI_SUM_MAX_TERMS || op->R > LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  if (!ski_sum_shape_ok(op->B, op->nterms, op->N, op->n2, op->R)) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

// the layout of the SKI kind (ski_interp_plan, then the Toeplitz partials) over the G = B P members
int ski_sum_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  if (const int rc = ski_sum_desc_check(&op)) return rc;
  if (pl->c > INT_MAX / LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  SkiPlan& k = pl->ski;
  const int64_t M = op.R, G = op.B * op.nterms;
  k.w = *op.interp;
  k.u = ar->take<float>((size_t)G * M * pl->c);
  k.t = ar->take<float>((size_t)G * M * pl->c);
  if (!ar->ok) return LO_ERR_WORKSPACE;
  if (k.w.right_plan) {  // the caller keeps the grid-major copy of W_r across calls (lo_interp_plan_build over G members)
    k.csr = csr_view(k.w.right_plan, G, op.N, op.n2, M);
  } else {
    const int rc = csr_build(k.w.right_idx, G, op.N, op.n2, M, ar, &k.csr, st);
    if (rc) return rc;
  }
  k.tz_part = ar->take<float>(toeplitz_part_floats(G, M, pl->c));
  return LO_OK;
}

int ski_sum_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const SkiPlan& k = pl->ski;
  const int64_t M = op.R, P = op.nterms, G = op.B * P;
  int rc = interp_scatter_bcast(k.csr.ptr, k.csr.ids, k.w.right_vals, G, (int)P, op.N, op.n2, M, v, pl->c, k.u, stop, st);
  if (!rc) rc = toeplitz_mv(op.A0, G, M, k.u, pl->c, nullptr, LO_DIAG_NONE, nullptr, k.t, k.tz_part, stop, st);
  if (!rc) rc = interp_sum(k.w.left_idx, k.w.left_vals, op.B, P, op.N, op.n2, M, k.t, pl->c, op.d, op.diag_mode, v, y,
                           stop, st);
  return rc;
}

}  // namespace lo

using namespace lo;

extern "C" {

int lo_interp_sum_f32(const int64_t* idx, const float* vals, int64_t B, int64_t P, int64_t N, int64_t J, int64_t M,
                      const float* u, int64_t c, const float* d, int32_t diag_mode, const float* v, float* y,
                      void* stream) {
  if (!idx || !vals || !u || !y || P < 1 || J < 1 || c < 1 || c > INT_MAX) return LO_ERR_BADARG;
  if (diag_mode != LO_DIAG_NONE && diag_mode != LO_DIAG_FULL && diag_mode != LO_DIAG_CONST) return LO_ERR_BADARG;
  if (diag_mode != LO_DIAG_NONE && (!d || !v)) return LO_ERR_BADARG;
  if (B < 1 || N < 1 || M < 1) return LO_ERR_BADARG;
  if (!ski_sum_shape_ok(B, P, N, J, M)) return LO_ERR_UNSUPPORTED;
  return interp_sum(idx, vals, B, P, N, J, M, u, c, d, diag_mode, v, y, nullptr, (hipStream_t)stream);
}

int lo_interp_t_bcast_planned_f32(const void* plan, const float* vals, int64_t B, int64_t P, int64_t N, int64_t J,
                                  int64_t M, const float* v, int64_t c, float* out, void* stream) {
  if (!plan || !vals || !v || !out || P < 1 || J < 1 || B < 1 || N < 1 || M < 1) return LO_ERR_BADARG;
  if (!ski_sum_shape_ok(B, P, N, J, M)) return LO_ERR_UNSUPPORTED;
  const CsrBufs b = csr_view(plan, B * P, N, J, M);
  return interp_scatter_bcast(b.ptr, b.ids, vals, B * P, (int)P, N, J, M, v, c, out, nullptr, (hipStream_t)stream);
}

}  // extern "C"
