// lo_masked.hip -- LO_OP_MASKED: y = S (base) S^T v + d o v, S selecting the rows idx [M] of a base operator of size N0
// (reference: MaskedLinearOperator._matmul masked_linear_operator.py:52-60 -- zeros, res[..., mask, :] = rhs, the base's
// _matmul, res[..., mask, :] -- whose two boolean indexings each run a nonzero, a device-to-host synchronisation, per
// product).  Here the index list is built once by the caller and the plan inverts it once.
//   generic route   k_mask_expand (u = S^T v, one coalesced write of u) -> matvec_run(base) -> k_mask_gather (+ d o v)
//   dense route     k_mask_expand -> k_masked_dense_mv: workgroups own blocks of SELECTED rows, row idx[i] of K is read
//                   in full against u, the base's diagonal enters as d0[idx[i]] v[i], y is written compact: M N0 floats
//                   of K instead of N0^2, no w, no gather pass.  The row product is k_dense_mv's (lo_dense.hip) with a
//                   row map; it is a kernel of its own so that the unmasked kernel's code object stays what it was.
// Plain streaming launches: no atomics, fixed summation order, bitwise reproducible.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

// inv[n] = position of n in idx, or -1: idx is strictly increasing, so every n finds its own answer by bisection -- no
// clearing pass, no scatter, and an idx entry outside [0, N0) is simply never found
__global__ __launch_bounds__(kThreads) void k_mask_inv(const int64_t* __restrict__ idx, int M, int* __restrict__ inv,
                                                        int N0) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N0) return;
  int lo = 0, hi = M;  // first position with idx[pos] >= n
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < (int64_t)n) lo = mid + 1;
    else hi = mid;
  }
  inv[n] = (lo < M && idx[lo] == (int64_t)n) ? lo : -1;
}

// u[b, n, :] = inv[n] >= 0 ? v[b, inv[n], :] : 0 -- four consecutive floats of u per lane, one 16-byte store
__global__ __launch_bounds__(kThreads) void k_mask_expand(const int* __restrict__ inv, const float* __restrict__ v,
                                                           float* __restrict__ u, int M, int N0, int c,
                                                           const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t tot = (size_t)N0 * c;
  const size_t e0 = 4 * ((size_t)blockIdx.x * kThreads + threadIdx.x);
  if (e0 >= tot) return;
  const float* vb = v + (size_t)blockIdx.y * M * c;
  float* ub = u + (size_t)blockIdx.y * tot;
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t e = e0 + q;
    float val = 0.f;
    if (e < tot) {
      const int n = (int)(e / c), k = (int)(e - (size_t)n * c);
      const int i = inv[n];
      if (i >= 0) val = vb[(size_t)i * c + k];
    }
    o[q] = val;
  }
  if ((tot & 3) == 0 && (reinterpret_cast<uintptr_t>(u) & 15) == 0) {  // every member's u starts on a 16-byte boundary
    *reinterpret_cast<float4*>(ub + e0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (e0 + q < tot) ub[e0 + q] = o[q];
  }
}

// y[b, i, :] = w[b, idx[i], :] + d-term(i) v[b, i, :]   (an index outside [0, N0) contributes nothing)
__global__ __launch_bounds__(kThreads) void k_mask_gather(const int64_t* __restrict__ idx, const float* __restrict__ w,
                                                           const float* __restrict__ dd, int dd_mode,
                                                           const float* __restrict__ v, float* __restrict__ y, int M,
                                                           int N0, int c, const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t tot = (size_t)M * c;
  const size_t e0 = 4 * ((size_t)blockIdx.x * kThreads + threadIdx.x);
  if (e0 >= tot) return;
  const int b = blockIdx.y;
  const float* wb = w + (size_t)b * N0 * c;
  const float* vb = v + (size_t)b * tot;
  float* yb = y + (size_t)b * tot;
  const float dc = (dd_mode == LO_DIAG_CONST) ? dd[b] : 0.f;
  float o[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t e = e0 + q;
    float val = 0.f;
    if (e < tot) {
      const int i = (int)(e / c), k = (int)(e - (size_t)i * c);
      const int64_t n = idx[i];
      if (n >= 0 && n < N0) val = wb[(size_t)n * c + k];
      if (dd_mode != LO_DIAG_NONE) {
        const float dv = (dd_mode == LO_DIAG_FULL) ? dd[(size_t)b * M + i] : dc;
        val = fmaf(dv, vb[e], val);
      }
    }
    o[q] = val;
  }
  if ((tot & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0) {
    *reinterpret_cast<float4*>(yb + e0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (e0 + q < tot) yb[e0 + q] = o[q];
  }
}

constexpr int kMaskRB = 4;  // rows per wave pass, as k_dense_mv

// One wave owns 4 selected rows at a time (register tile 4 rows x CT columns), lanes stride over the N0 columns of the
// rows idx[i] of K, 16 bytes per lane when the rows are 16-byte aligned (N0 % 4 == 0), else a scalar path; u is
// re-read through L1 / L2 like k_dense_mv's v.  Epilogue: + d0[idx[i]] v[i] (the base's diagonal) + d[i] v[i].
template <int CT>
__global__ __launch_bounds__(kThreads) void k_masked_dense_mv(
    const float* __restrict__ K, const int64_t* __restrict__ idx, const float* __restrict__ d0, int d0_mode,
    const float* __restrict__ dd, int dd_mode, const float* __restrict__ u, const float* __restrict__ v, int ldv, int c,
    float* __restrict__ y, int M, int N0, int rows_per_wg, const int* __restrict__ stop) {
  if (stop && *stop) return;
  const int s = blockIdx.x, b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rows_per_wave = rows_per_wg / 4;
  const int wr0 = s * rows_per_wg + wave * rows_per_wave;
  const int wr1 = min(M, wr0 + rows_per_wave);
  const float* Kb = K + (size_t)b * N0 * N0;
  const float* ub = u + (size_t)b * N0 * ldv;
  const float* vb = v + (size_t)b * M * ldv;
  float* yb = y + (size_t)b * M * ldv;
  const float dc = (dd_mode == LO_DIAG_CONST) ? dd[b] : 0.f;
  const float d0c = (d0_mode == LO_DIAG_CONST) ? d0[b] : 0.f;
  const int N4 = N0 & ~3;

  for (int row = wr0; row < wr1; row += kMaskRB) {
    float acc[kMaskRB][CT];
#pragma unroll
    for (int r = 0; r < kMaskRB; ++r)
#pragma unroll
      for (int k = 0; k < CT; ++k) acc[r][k] = 0.f;
    const float* kr[kMaskRB];
    int64_t src[kMaskRB];
#pragma unroll
    for (int r = 0; r < kMaskRB; ++r) {
      src[r] = idx[min(row + r, M - 1)];
      const bool in = src[r] >= 0 && src[r] < N0;
      if (!in) src[r] = -1;
      kr[r] = Kb + (size_t)(in ? src[r] : 0) * N0;  // (a row outside the base is read as row 0 and dropped below)
    }

    if ((N0 & 3) == 0) {
      for (int j = 4 * lane; j < N4; j += 256) {
        float4 a[kMaskRB];
#pragma unroll
        for (int r = 0; r < kMaskRB; ++r) a[r] = *reinterpret_cast<const float4*>(kr[r] + j);
        float vv[4][CT];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int k = 0; k < CT; ++k) vv[jj][k] = (k < c) ? ub[(size_t)(j + jj) * ldv + k] : 0.f;
#pragma unroll
        for (int r = 0; r < kMaskRB; ++r)
#pragma unroll
          for (int k = 0; k < CT; ++k) {
            float t = acc[r][k];
            t = fmaf(a[r].x, vv[0][k], t);
            t = fmaf(a[r].y, vv[1][k], t);
            t = fmaf(a[r].z, vv[2][k], t);
            t = fmaf(a[r].w, vv[3][k], t);
            acc[r][k] = t;
          }
      }
    } else {  // rows of K start on 4-byte boundaries only
      for (int j = lane; j < N0; j += 64) {
#pragma unroll
        for (int r = 0; r < kMaskRB; ++r) {
          const float a = kr[r][j];
#pragma unroll
          for (int k = 0; k < CT; ++k) acc[r][k] = fmaf(a, (k < c) ? ub[(size_t)j * ldv + k] : 0.f, acc[r][k]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kMaskRB; ++r)
#pragma unroll
      for (int k = 0; k < CT; ++k) acc[r][k] = wave_sum(acc[r][k]);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kMaskRB; ++r) {
        const int rr = row + r;
        if (rr < wr1) {
          const bool in = src[r] >= 0;
          const float dv = (dd_mode == LO_DIAG_FULL) ? dd[(size_t)b * M + rr] : dc;
          const float d0v = !in ? 0.f : (d0_mode == LO_DIAG_FULL) ? d0[(size_t)b * N0 + src[r]] : d0c;
#pragma unroll
          for (int k = 0; k < CT; ++k) {
            if (k < c) {
              const float vin = vb[(size_t)rr * ldv + k];
              const float kv = in ? acc[r][k] : 0.f;
              yb[(size_t)rr * ldv + k] = fmaf(dv, vin, fmaf(d0v, vin, kv));
            }
          }
        }
      }
    }
  }
}

static bool mask_base_ok(const lo_op_desc* base) {
  if (base->kind == LO_OP_SUM && base->terms)  // (a sum's kernel terms are not taken under a mask)
    for (int i = 0; i < base->nterms && i < LO_MAX_TERMS; ++i)
      if (kernel_term_kind(base->terms[i].kind)) return false;
  return plain_term_kind(base->kind) || base->kind == LO_OP_SUM;
}

// the dense route: a dense base at the column counts the vector-ALU k_dense_mv takes (the matrix-core engine of wider
// blocks reads whole tiles of K; those go the generic way round it)
static bool mask_dense_route(const lo_op_desc* base, int64_t c) {
  return base->kind == LO_OP_DENSE_DIAG && !dense_mfma_ok(base->N, c);
}

static int mask_check(const lo_op_desc* op) {
  const lo_mask_desc* m = op->mask;
  if (!m || !m->base || !m->idx) return LO_ERR_BADARG;
  if (!mask_base_ok(m->base)) return LO_ERR_UNSUPPORTED;
  if (m->M != op->N || m->base->B != op->B || m->base->N < 1) return LO_ERR_BADARG;
  if (m->base->N > 0x7ffffff0 || m->M > 0x7ffffff0) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

static Split mask_base_split(const lo_op_desc* base) { return choose_split(base->B, base->N, 256); }

int masked_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  int rc = mask_check(&op);
  if (rc) return rc;
  const lo_mask_desc* m = op.mask;
  const lo_op_desc* base = m->base;
  MaskedPlan& k = pl->mask;
  k.idx = m->idx;
  k.N0 = base->N;
  k.dense = mask_dense_route(base, pl->c);
  k.inv = ar->take<int>((size_t)base->N);
  k.u = ar->take<float>((size_t)base->B * base->N * pl->c);
  k.w = k.dense ? nullptr : ar->take<float>((size_t)base->B * base->N * pl->c);
  MatvecPlan scratch;  // (a measuring pass keeps no sub-plan)
  MatvecPlan* sub = &scratch;
  if (!ar->measuring()) {
    sub = pl->sub = new MatvecPlan[1]();
    pl->nterms = 1;
  }
  rc = matvec_plan_init(sub, base, nullptr, nullptr, pl->c, mask_base_split(base), ar, st);
  if (rc || ar->measuring()) return rc;
  if (!ar->ok) return LO_ERR_WORKSPACE;
  // streaming kernels only for a low-rank base (its one-pass product is a resident launch); the terms of a sum base keep
  // their own choice
  if (base->kind == LO_OP_LOWRANK_DIAG) sub->lr.mv_resident = false;
  hipLaunchKernelGGL(k_mask_inv, dim3((unsigned)((base->N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, m->idx,
                     (int)m->M, k.inv, (int)base->N);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int masked_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const lo_op_desc& base = pl->sub[0].op;
  const MaskedPlan& k = pl->mask;
  const int M = (int)op.N, N0 = (int)k.N0, c = (int)pl->c;
  const dim3 block(kThreads);
  const size_t per = (size_t)4 * kThreads;
  LO_PROF_BEGIN("mask_expand", st);
  hipLaunchKernelGGL(k_mask_expand, dim3((unsigned)(((size_t)N0 * c + per - 1) / per), (unsigned)op.B), block, 0, st,
                     k.inv, v, k.u, M, N0, c, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (k.dense) {
    const int rows_per_wg = dense_rows_per_wg(op.B, M);
    const dim3 grid((unsigned)((M + rows_per_wg - 1) / rows_per_wg), (unsigned)op.B);
    for (int c0 = 0; c0 < c; c0 += 4) {
      const int cn = std::min(4, c - c0);
#define LO_MDM(CT)                                                                                                  \
  hipLaunchKernelGGL((k_masked_dense_mv<CT>), grid, block, 0, st, base.A0, k.idx, base.d, base.diag_mode, op.d, \
                     op.diag_mode, k.u + c0, v + c0, c, cn, y + c0, M, N0, rows_per_wg, stop)
      LO_PROF_BEGIN("masked_dense_mv", st);
      if (cn == 1) LO_MDM(1);
      else if (cn == 2) LO_MDM(2);
      else LO_MDM(4);
#undef LO_MDM
      LO_PROF_END(st);
      LO_LAUNCH_CHECK();
    }
    return LO_OK;
  }
  const int rc = matvec_run(&pl->sub[0], k.u, k.w, nullptr, stop, st);
  if (rc) return rc;
  LO_PROF_BEGIN("mask_gather", st);
  hipLaunchKernelGGL(k_mask_gather, dim3((unsigned)(((size_t)M * c + per - 1) / per), (unsigned)op.B), block, 0, st,
                     k.idx, k.w, op.d, op.diag_mode, v, y, M, N0, c, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// u = S^T v alone (the operator's _bilinear_derivative expands both vector blocks before the base's contraction)
int masked_expand(const int64_t* idx, int64_t M, int64_t N0, const float* v, float* u, int* inv, int64_t B, int64_t c,
                  hipStream_t st) {
  hipLaunchKernelGGL(k_mask_inv, dim3((unsigned)((N0 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, idx, (int)M,
                     inv, (int)N0);
  LO_LAUNCH_CHECK();
  const size_t per = (size_t)4 * kThreads;
  hipLaunchKernelGGL(k_mask_expand, dim3((unsigned)(((size_t)N0 * c + per - 1) / per), (unsigned)B), dim3(kThreads), 0,
                     st, inv, v, u, (int)M, (int)N0, (int)c, nullptr);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_mask_expand_workspace_bytes(int64_t N0) { return align_up((size_t)std::max<int64_t>(N0, 1) * sizeof(int), 256); }

int lo_mask_expand_f32(const int64_t* idx, int64_t M, int64_t N0, const float* v, float* u, int64_t B, int64_t c,
                       void* ws, size_t ws_bytes, void* stream) {
  if (!idx || !v || !u || M < 1 || N0 < 1 || B < 1 || c < 1) return LO_ERR_BADARG;
  if (N0 > 0x7ffffff0 || M > 0x7ffffff0) return LO_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < lo_mask_expand_workspace_bytes(N0)) return LO_ERR_WORKSPACE;
  return masked_expand(idx, M, N0, v, u, (int*)ws, B, c, (hipStream_t)stream);
}

}  // extern "C"
