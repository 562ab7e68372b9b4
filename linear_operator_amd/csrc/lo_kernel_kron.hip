// lo_kernel_kron.hip -- the matrix-free multitask operator K(X, X) (x) Bt, LO_OP_KERNEL_KRON_DIAG and the entry point
// lo_kernel_kron_mv_f32 of lo_amd.h (the reference's MultitaskKernel returns KroneckerProductLinearOperator(covar_x,
// covar_task), kronecker_product_linear_operator.py:34-45; here neither K nor the product is ever in memory).
//
// Row and column index i T + t, the data index slowest.  With y and v viewed as [B, n, T c] ("wide" column w = t c + col)
//   y[i, t c + col] = theta_D sum_j g(r_ij) w[j, t c + col] + d o v,   w[j, t c + col] = sum_s Bt[t, s] v[j, s c + col]
// so the product is the sweep of k_kernel_mv (lo_kernel_op.hip) over the n points with T c columns: a workgroup owns 256
// data rows i, one per thread, x2 is scaled while it is staged in tiles of 128, every lane reads the same LDS entry
// (broadcast), r^2 by direct differences, a tile's sums formed on their own and then added to the running ones.  What
// differs: Bt (<= 64 floats) sits in LDS and is applied while the tile of v is staged (sum over s ascending, one FMA
// chain), a pair carries up to 32 wide accumulators (T c is never narrow: 68 for 17 columns at T = 4, and every sweep
// recomputes the exponentials), and the store addresses row i T + t with the diagonal indexed by the full row.
// Few rows: the columns j are split as in ko_shape, the partials [js, B, n, T c] are added in ascending order by
// k_kernel_mv_reduce, which also applies + d o v.  No atomics, no workgroup waits for another: two calls give equal bits.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"

namespace lo {

// (the task count, the shape bounds and the wide column chunk of a sweep -- kk_tasks_ok, kk_shape_ok, kk_col_chunk /
// kk_cols: lo_kernel_shape.h)

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, n, T c]
template <int FAMILY, int DP, int CCW>
__global__ __launch_bounds__(kThreads) void k_kernel_kron_mv(const float* __restrict__ x, const float* __restrict__ theta,
                                                             const float* __restrict__ task, int n, int D, int T,
                                                             const float* __restrict__ v, int c,
                                                             const float* __restrict__ dd_ptr, int dd_mode,
                                                             float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                             const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float ws[kKoTJ * CCW];
  __shared__ float th[DP];
  __shared__ float bt[LO_KERNEL_KRON_MAX_TASKS * LO_KERNEL_KRON_MAX_TASKS];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;
  const int W = T * c;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0f;
  if ((int)threadIdx.x < T * T) bt[threadIdx.x] = task[b * T * T + threadIdx.x];
  __syncthreads();
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x[((size_t)b * n + i) * D + k] * th[k] : 0.0f;
  const float os2 = theta[b * (D + 1) + D];
  const float* xb = x + (size_t)b * n * D;
  const float* vb = v + (size_t)b * n * W;
  const int j0 = blockIdx.z * jchunk, j1 = min(n, j0 + jchunk);
  for (int w0 = 0; w0 < W; w0 += CCW) {
    float acc[CCW];
#pragma unroll
    for (int cc = 0; cc < CCW; ++cc) acc[cc] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
        const int j = e / DP, dd = e - j * DP;
        xs[e] = dd < D ? xb[(size_t)(jt + j) * D + dd] * th[dd] : 0.0f;
      }
      for (int e = threadIdx.x; e < nj * CCW; e += kThreads) {  // the task factor applied on the way in
        const int j = e / CCW, w = w0 + (e - j * CCW);
        float r = 0.0f;
        if (w < W) {
          const int t = w / c, col = w - t * c;
          const float* vj = vb + (size_t)(jt + j) * W + col;
          for (int s = 0; s < T; ++s) r = fmaf(bt[t * T + s], vj[(size_t)s * c], r);
        }
        ws[e] = r;
      }
      __syncthreads();
      float tacc[CCW];
#pragma unroll
      for (int cc = 0; cc < CCW; ++cc) tacc[cc] = 0.0f;
#pragma unroll 2
      for (int j = 0; j < nj; ++j) {
        float r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float df = a[k] - xs[j * DP + k];
          r2 = fmaf(df, df, r2);
        }
        const float kv = kf_g<FAMILY>(r2);
#pragma unroll
        for (int cc = 0; cc < CCW; ++cc) tacc[cc] = fmaf(kv, ws[j * CCW + cc], tacc[cc]);
      }
#pragma unroll
      for (int cc = 0; cc < CCW; ++cc) acc[cc] += tacc[cc];
    }
    if (live) {
#pragma unroll
      for (int cc = 0; cc < CCW; ++cc) {
        const int w = w0 + cc;
        if (w < W) {
          const size_t o = ((size_t)b * n + i) * W + w;  // = (row i T + t) c + col of [B, n T, c]
          float r = os2 * acc[cc];
          if (part) {
            part[(size_t)blockIdx.z * gridDim.y * n * W + o] = r;
          } else {
            if (dd_mode == LO_DIAG_FULL) r = fmaf(dd_ptr[((size_t)b * n + i) * T + w / c], v[o], r);
            else if (dd_mode == LO_DIAG_CONST) r = fmaf(dd_ptr[b], v[o], r);
            y[o] = r;
          }
        }
      }
    }
  }
}

// the product on validated arguments; part: the partials [js, B, n, T c] of a split member (ko_split_layout)
static int kk_mv_run(const float* x, const float* theta, const float* task, int family, int64_t B, int64_t n, int64_t D,
                     int64_t T, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                     const int* stop, hipStream_t st) {
  const KoSweep w(B, n, n, D);
  const int64_t W = T * c;
  float* p = w.s.js > 1 ? part : nullptr;
  LO_PROF_BEGIN("k_kernel_kron_mv", st);
  ko_dispatch(family, w.DP, kk_cols{}, kk_col_chunk(W), [&](auto F, auto P, auto C) {
    hipLaunchKernelGGL((k_kernel_kron_mv<F(), P(), C()>), w.grid, dim3(kThreads), 0, st, x, theta, task, (int)n, (int)D,
                       (int)T, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)  // (rows of c elements: the full diagonal of the reduction is indexed by o / c = the full row i T + t)
    return ko_reduce_splits("k_kernel_kron_mv_reduce", p, w.s.js, (size_t)n * W, (size_t)B * n * W, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

int kernel_kron_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || !op->task || op->R < 1 || !ko_family_ok(op->n2) || op->nterms < 1) return LO_ERR_BADARG;
  if (op->N < 1 || op->N % op->nterms != 0) return LO_ERR_BADARG;
  if (op->R > LO_KERNEL_MAX_DIM || op->nterms > LO_KERNEL_KRON_MAX_TASKS) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

int kernel_kron_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_kron_desc_check(&op)) return rc;
  const int64_t n = op.N / op.nterms;
  if (!kk_shape_ok(op.B, n, op.R, op.nterms, pl->c)) return LO_ERR_UNSUPPORTED;
  pl->kk.part = ko_split_layout<float>(*ar, op.B, n, n, op.nterms * pl->c);
  return LO_OK;
}

int kernel_kron_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return kk_mv_run(op.A0, op.A1, op.task, (int)op.n2, op.B, op.N / op.nterms, op.R, op.nterms, v, pl->c, op.d,
                   op.diag_mode, y, pl->kk.part, stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_kron_mv_workspace_bytes(int64_t B, int64_t n, int64_t D, int64_t T, int64_t c) {
  if (!ko_args_ok(B, n, n, D, c) || !kk_tasks_ok(T) || !kk_shape_ok(B, n, D, T, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, n, n, T * c); });
}

int lo_kernel_kron_mv_f32(const float* x, const float* theta, const float* task, int32_t family, int64_t B, int64_t n,
                          int64_t D, int64_t T, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!x || !theta || !task || !v || !y || !ko_args_ok(B, n, n, D, c) || !ko_family_ok(family) || T < 1)
    return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, true)) return LO_ERR_BADARG;  // (the operator is square: d whenever a mode is given)
  if (!kk_tasks_ok(T) || !kk_shape_ok(B, n, D, T, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, n, n, T * c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kk_mv_run(x, theta, task, family, B, n, D, T, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

}  // extern "C"

