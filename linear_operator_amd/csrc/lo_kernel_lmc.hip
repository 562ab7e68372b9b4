// lo_kernel_lmc.hip -- the matrix-free linear model of coregionalisation sum_q K_q(X, X) (x) B_q, LO_OP_KERNEL_LMC_DIAG and
// the entry point lo_kernel_lmc_mv_f32 of lo_amd.h (the reference's LCMKernel returns a SumLinearOperator of
// KroneckerProductLinearOperator(covar_x_q, covar_task_q); here neither a K_q nor a product is ever in memory).
//
// Row and column index i T + t, the data index slowest.  With y and v viewed as [B, n, T c] ("wide" column w = t c + col)
//   y[i, w] = sum_q os2_q sum_j g_{f_q}(r_q,ij) w_q[j, w] + d o v,   w_q[j, t c + col] = sum_s B_q[t, s] v[j, s c + col]
// The sweep is that of k_kernel_kron_mv (lo_kernel_kron.hip): a workgroup owns 256 data rows i, one per thread, tiles of
// x2 and of v stream through LDS, every lane reads the same LDS entry (broadcast), r^2 by direct differences, a tile's
// sums formed on their own and then added to the running ones.  The per-term pieces are those of lo_kernel_sum.hip
// (lo_kernel_terms.h): the tile of x2 is staged once PER TERM, scaled by that term's inverse lengthscales through the
// same rounding as the thread's own point (ks_scale: coincident points give r = 0), and a tile is walked in sub-tiles of
// 8 pairs with the term loop OUTSIDE the sub-tile, so a term's family is switched on once per 8 pairs.
//
// The task factors are applied on the way IN: while the tile of v is staged, every term's w_q = B_q v is formed (sum over
// s ascending, one FMA chain) into its own copy of the tile, Q copies [Q][TJ][CCW] in LDS, and a thread carries ONE set
// of wide accumulators: per sub-tile and term kv[8] = os2_q g_q(r_q), then acc[w] += kv[jj] w_q[jj][w].  The other way --
// v staged once, Q sets of accumulators z_q, y = sum_q os2_q B_q z_q at the store -- needs 2 Q CCW registers a thread (a
// tile's sums and the running ones per term) where this needs 2 CCW, and the T^2 Q products per row at the store; the Q
// B_q v products here are formed once per tile by 256 threads for the 256 rows that read them.  LDS: Q TJ (DP + CCW)
// floats, so the point tile halves at DP = 32 (ks_tile) and three or four terms carry 8 wide columns per sweep, one or
// two 16 (kl_col_chunk): 50.4 KB at the most.  Columns beyond that take further sweeps; rows of a ragged last sub-tile
// are staged as zeros (points and w_q): they add exactly 0.
// Few rows: the points j are split as in ko_shape, the partials [js, B, n, T c] are added in ascending order by
// k_kernel_mv_reduce, which also applies + d o v.  No atomics, no workgroup waits for another: two calls give equal bits.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_terms.h"

namespace lo {

static bool kl_terms_ok(int64_t Q) { return Q >= 1 && Q <= LO_KERNEL_MAX_TERMS; }

static size_t kl_lds_bytes(int Q, int DP, int T, int CCW) {
  const int TJ = DP == 32 ? kKoTJ / 2 : kKoTJ;  // (ks_tile<DP>())
  return ((size_t)Q * TJ * (DP + CCW) + (size_t)Q * (DP + 1) + (size_t)Q * T * T) * sizeof(float);
}

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, n, T c].
// `fams`: the family codes, four bits per term, term 0 lowest.  Dynamic LDS: kl_lds_bytes(Q, DP, T, CCW)
template <int DP, int CCW>
__global__ __launch_bounds__(kThreads) void k_kernel_lmc_mv(const float* __restrict__ x, const float* __restrict__ theta,
                                                            const float* __restrict__ task, unsigned fams, int Q, int n,
                                                            int D, int T, const float* __restrict__ v, int c,
                                                            const float* __restrict__ dd_ptr, int dd_mode,
                                                            float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                            const int* __restrict__ stop) {
  if (stop && *stop) return;
  extern __shared__ __align__(16) float kl_smem[];
  constexpr int TJ = ks_tile<DP>();
  float* xs = kl_smem;                     // [Q][TJ][DP]
  float* ws = xs + (size_t)Q * TJ * DP;    // [Q][TJ][CCW]
  float* th = ws + (size_t)Q * TJ * CCW;   // [Q][DP + 1]
  float* bt = th + Q * (DP + 1);           // [Q][T][T]
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < n;
  const int W = T * c;
  ks_stage_theta<DP>(theta + (size_t)b * Q * (D + 1), D, 0, Q, th);
  for (int e = threadIdx.x; e < Q * T * T; e += kThreads) bt[e] = task[(size_t)b * Q * T * T + e];
  __syncthreads();
  float araw[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) araw[k] = (live && k < D) ? x[((size_t)b * n + i) * D + k] : 0.0f;
  const float* xb = x + (size_t)b * n * D;
  const float* vb = v + (size_t)b * n * W;
  const int j0 = blockIdx.z * jchunk, j1 = min(n, j0 + jchunk);
  for (int w0 = 0; w0 < W; w0 += CCW) {
    float acc[CCW];
#pragma unroll
    for (int cc = 0; cc < CCW; ++cc) acc[cc] = 0.0f;
    for (int jt = j0; jt < j1; jt += TJ) {
      const int nj = min(TJ, j1 - jt);
      const int njp = (nj + kKsJS - 1) / kKsJS * kKsJS;
      __syncthreads();  // (the previous tile has been read)
      ks_stage_points<DP>(xb, th, D, Q, jt, nj, njp, xs);
      const int per = njp * CCW;
      for (int e = threadIdx.x; e < Q * per; e += kThreads) {  // every term's task factor applied on the way in
        const int q = e / per, r = e - q * per;
        const int j = r / CCW, w = w0 + (r - j * CCW);
        float s = 0.0f;
        if (j < nj && w < W) {
          const int t = w / c, col = w - t * c;
          const float* vj = vb + (size_t)(jt + j) * W + col;
          const float* bq = bt + (q * T + t) * T;
          for (int ss = 0; ss < T; ++ss) s = fmaf(bq[ss], vj[(size_t)ss * c], s);
        }
        ws[((size_t)q * TJ + j) * CCW + (r - j * CCW)] = s;
      }
      __syncthreads();
      float tacc[CCW];
#pragma unroll
      for (int cc = 0; cc < CCW; ++cc) tacc[cc] = 0.0f;
      for (int js = 0; js < njp; js += kKsJS) {
        for (int q = 0; q < Q; ++q) {
          float at[DP], kv[kKsJS];
#pragma unroll
          for (int k = 0; k < DP; ++k) at[k] = ks_scale(araw[k], th[q * (DP + 1) + k]);
#pragma unroll
          for (int jj = 0; jj < kKsJS; ++jj) kv[jj] = 0.0f;
          const float os2 = th[q * (DP + 1) + DP];
          const float* xt = xs + ((size_t)q * TJ + js) * DP;
#define KL_CALL(F_) ks_sub_g<F_, DP>(at, xt, os2, kv)
          KS_FAMILY_SWITCH((fams >> (4 * q)) & 15u, KL_CALL)
#undef KL_CALL
          const float* wq = ws + ((size_t)q * TJ + js) * CCW;
#pragma unroll
          for (int jj = 0; jj < kKsJS; ++jj) {
#pragma unroll
            for (int cc = 0; cc < CCW; ++cc) tacc[cc] = fmaf(kv[jj], wq[jj * CCW + cc], tacc[cc]);
          }
        }
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
          float r = acc[cc];
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

// the descriptor's n2: the Q family codes in the low 16 bits (four per term, term 0 lowest), Q in bits 16 .. 19
static int64_t kl_desc_terms(int64_t n2) { return (n2 >> 16) & 15; }
static unsigned kl_desc_fams(int64_t n2) { return (unsigned)(n2 & 0xffff); }
// four known codes, and none set beyond the Q terms (Q >= 1)
static bool kl_fams_ok(int64_t fams, int64_t Q) {
  if (fams < 0 || fams > 0xffff) return false;
  for (int t = 0; t < LO_KERNEL_MAX_TERMS; ++t) {
    const int64_t f = (fams >> (4 * t)) & 15;
    if (!ko_family_ok(f) || (t >= Q && f != 0)) return false;
  }
  return true;
}

// the product on validated arguments; part: the partials [js, B, n, T c] of a split member (ko_split_layout)
static int kl_mv_run(const float* x, const float* theta, const float* task, unsigned fams, int64_t B, int64_t n, int64_t D,
                     int64_t Q, int64_t T, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                     const int* stop, hipStream_t st) {
  const KoSweep w(B, n, n, D);
  const int64_t W = T * c;
  const int CCW = kl_col_chunk(Q, W);
  const size_t lds = kl_lds_bytes((int)Q, w.DP, (int)T, CCW);
  float* p = w.s.js > 1 ? part : nullptr;
  LO_PROF_BEGIN("k_kernel_lmc_mv", st);
  ko_pick(ko_dims{}, w.DP, [&](auto P) {
    ko_pick(kl_cols{}, CCW, [&](auto C) {
      hipLaunchKernelGGL((k_kernel_lmc_mv<P(), C()>), w.grid, dim3(kThreads), lds, st, x, theta, task, fams, (int)Q, (int)n,
                         (int)D, (int)T, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)  // (rows of c elements: the full diagonal of the reduction is indexed by o / c = the full row i T + t)
    return ko_reduce_splits("k_kernel_lmc_mv_reduce", p, w.s.js, (size_t)n * W, (size_t)B * n * W, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

int kernel_lmc_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || !op->task || op->R < 1 || op->nterms < 1) return LO_ERR_BADARG;
  if (op->n2 < 0 || (op->n2 >> 20) != 0 || kl_desc_terms(op->n2) < 1) return LO_ERR_BADARG;
  if (!kl_fams_ok(kl_desc_fams(op->n2), kl_desc_terms(op->n2))) return LO_ERR_BADARG;
  if (op->N < 1 || op->N % op->nterms != 0) return LO_ERR_BADARG;
  if (op->R > LO_KERNEL_MAX_DIM || !kk_tasks_ok(op->nterms) || !kl_terms_ok(kl_desc_terms(op->n2)))
    return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

int kernel_lmc_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_lmc_desc_check(&op)) return rc;
  const int64_t n = op.N / op.nterms;
  if (!kk_shape_ok(op.B, n, op.R, op.nterms, pl->c)) return LO_ERR_UNSUPPORTED;
  pl->kk.part = ko_split_layout<float>(*ar, op.B, n, n, op.nterms * pl->c);
  return LO_OK;
}

int kernel_lmc_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return kl_mv_run(op.A0, op.A1, op.task, kl_desc_fams(op.n2), op.B, op.N / op.nterms, op.R, kl_desc_terms(op.n2),
                   op.nterms, v, pl->c, op.d, op.diag_mode, y, pl->kk.part, stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_lmc_mv_workspace_bytes(int64_t B, int64_t n, int64_t D, int64_t Q, int64_t T, int64_t c) {
  if (!ko_args_ok(B, n, n, D, c) || !kl_terms_ok(Q) || !kk_tasks_ok(T) || !kk_shape_ok(B, n, D, T, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, n, n, T * c); });
}

int lo_kernel_lmc_mv_f32(const float* x, const float* theta, const float* task, int32_t families, int64_t B, int64_t n,
                         int64_t D, int64_t Q, int64_t T, const float* v, int64_t c, const float* d, int32_t diag_mode,
                         float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !theta || !task || !v || !y || !ko_args_ok(B, n, n, D, c) || Q < 1 || T < 1 || !kl_fams_ok(families, Q))
    return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, true)) return LO_ERR_BADARG;  // (the operator is square: d whenever a mode is given)
  if (!kl_terms_ok(Q) || !kk_tasks_ok(T) || !kk_shape_ok(B, n, D, T, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, n, n, T * c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kl_mv_run(x, theta, task, (unsigned)families, B, n, D, Q, T, v, c, d, diag_mode, y, part, nullptr,
                   (hipStream_t)stream);
}

}  // extern "C"
