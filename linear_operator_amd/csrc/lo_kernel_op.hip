// lo_kernel_op.hip -- the matrix-free kernel operator K(x1, x2)_ij = os2 g(|(x1_i - x2_j) / l|), LO_OP_KERNEL_DIAG and the
// entry points lo_kernel_mv_f32 / lo_kernel_bilinear_f32 / lo_kernel_points_grad_f32 of lo_amd.h (kernel_linear_operator.py:379-383 of the reference
// evaluates covar_func densely inside _matmul; here K is never in memory).
//
// Product (k_kernel_mv): a workgroup owns 256 rows i of one member, one per thread.  The thread scales its point once,
//   a_d = x1[i, d] theta[d] (theta = inverse lengthscales), and keeps it in DP registers next to CC column accumulators.
//   The points x2_j, scaled the same way while they are staged, and the rows v[j, c0 .. c0 + CC) stream through LDS in
//   tiles of 128; every lane reads the same tile entry, so the LDS reads are broadcasts without bank conflicts.  Per pair:
//   r^2 = sum_d (a_d - b_d)^2 by direct differences (never |a|^2 + |b|^2 - 2 a.b, which cancels for near points), g(r)
//   with one v_exp_f32 on a pre-multiplied argument (and one v_sqrt_f32 for the Matern families), CC FMAs.  A tile's sum is
//   formed on its own and then added to the running one (two-level summation).  More than CC columns: another sweep.
//   Ragged M, N, D, c are predicated: padded coordinates are 0 on both sides, rows beyond M compute and store nothing.
// Few rows (B ceil(M / 256) < 512 workgroups): the columns j are split over gridDim.z workgroups, the partials go to the
//   workspace and k_kernel_mv_reduce adds them in ascending order and applies + d o v.  No workgroup waits for another.
// Derivative (k_kernel_bil): the same sweep with W_ij = sum_s U[i, s] V[j, s] (8 columns s per sweep) in place of v, the
//   thread accumulating sum_j W_ij h(r) (a_d - b_d)^2 per dimension and sum_j W_ij g(r); one partial per workgroup by a
//   fixed-order block sum, k_kernel_bil_reduce adds them in ascending order.  No float atomics anywhere.
// Points (k_kernel_pgrad, lo_kernel_points_grad_f32): the same sweep once more, the thread accumulating
//   sum_j W_ij h(r) (a_d - b_d) per dimension for ITS row -- d / d x1[i, d] up to the factor theta_D theta_d; no sum across
//   threads.  The x2 side is the same kernel with the roles of x1 / x2 and U / V swapped.  Split columns as in the product.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c].
// tstride: floats between the thetas of two members (D + 1; T (D + 1) for one term of a [B, T, D + 1] array)
template <int FAMILY, int DP, int CC>
__global__ __launch_bounds__(kThreads) void k_kernel_mv(const float* __restrict__ x1, const float* __restrict__ x2,
                                                        const float* __restrict__ theta, int tstride, int M, int N, int D,
                                                        const float* __restrict__ v, int c,
                                                        const float* __restrict__ dd_ptr, int dd_mode,
                                                        float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                        const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * CC];
  __shared__ float th[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * tstride + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
  const float os2 = theta[b * tstride + D];
  const float* x2b = x2 + (size_t)b * N * D;
  const float* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += CC) {
    float acc[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * CC; e += kThreads) {
        const int j = e / CC, cc = e - j * CC;
        vs[e] = c0 + cc < c ? vb[(size_t)(jt + j) * c + c0 + cc] : 0.0f;
      }
      __syncthreads();
      float tacc[CC];
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) tacc[cc] = 0.0f;
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
        for (int cc = 0; cc < CC; ++cc) tacc[cc] = fmaf(kv, vs[j * CC + cc], tacc[cc]);
      }
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) acc[cc] += tacc[cc];
    }
    if (live) {
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) {
        const int col = c0 + cc;
        if (col < c) {
          const size_t o = ((size_t)b * M + i) * c + col;
          float r = os2 * acc[cc];
          if (part) {
            part[(size_t)blockIdx.z * gridDim.y * M * c + o] = r;
          } else {
            if (dd_mode == LO_DIAG_FULL) r = fmaf(dd_ptr[(size_t)b * M + i], v[o], r);
            else if (dd_mode == LO_DIAG_CONST) r = fmaf(dd_ptr[b], v[o], r);
            y[o] = r;
          }
        }
      }
    }
  }
}

// y[b, i, col] = sum_z part[z, b, i, col] (ascending z) + d o v; one thread per output element
__global__ __launch_bounds__(kThreads) void k_kernel_mv_reduce(const float* __restrict__ part, int js, size_t per_member,
                                                               size_t total, int c, const float* __restrict__ dd_ptr,
                                                               int dd_mode, const float* __restrict__ v,
                                                               float* __restrict__ y, const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= total) return;
  float r = part[o];
  for (int z = 1; z < js; ++z) r += part[(size_t)z * total + o];
  if (dd_mode == LO_DIAG_FULL) r = fmaf(dd_ptr[o / c], v[o], r);
  else if (dd_mode == LO_DIAG_CONST) r = fmaf(dd_ptr[o / per_member], v[o], r);
  y[o] = r;
}

// grid (row blocks, B, js); part [B, nblk = gridDim.x * gridDim.z, DP + 1]
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kernel_bil(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ theta, int M, int N, int D,
                                                         const float* __restrict__ U, const float* __restrict__ V, int t,
                                                         float* __restrict__ part, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ float th[DP];
  __shared__ float red[4];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
    gacc[k] = 0.0f;
  }
  float gos = 0.0f, gos_c = 0.0f;
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * kKoTS; e += kThreads) {
        const int j = e / kKoTS, ss = e - j * kKoTS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      float tacc[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float sd[DP];
        float r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          sd[k] = a[k] - xs[j * DP + k];
          r2 = fmaf(sd[k], sd[k], r2);
        }
        float g, h;
        kf_gh<FAMILY>(r2, &g, &h);
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
        {  // the outputscale entry is ONE number per member, a sum of N M terms of both signs: compensated (Kahan)
          const float term = fmaf(w, g, -gos_c);
          const float next = gos + term;
          gos_c = (next - gos) - term;
          gos = next;
        }
        const float wh = w * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh * sd[k], sd[k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
  float* out = part + ((size_t)b * nblk + blk) * (DP + 1);
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gacc[k], red);
    if (threadIdx.x == 0) out[k] = sum;
  }
  const float sum = block_sum256(gos, red);
  if (threadIdx.x == 0) out[DP] = sum;
}

// g_theta[b, q] from the nblk partials in ascending order: q < D: os2 / theta[q] times the sum, q == D: the sum
__global__ __launch_bounds__(64) void k_kernel_bil_reduce(const float* __restrict__ part, int nblk, int DP, int D,
                                                          const float* __restrict__ theta, float* __restrict__ g_theta) {
  const int64_t b = blockIdx.x;
  const int q = threadIdx.x;
  if (q > D) return;
  const int slot = q < D ? q : DP;
  const float* p = part + (size_t)b * nblk * (DP + 1) + slot;
  float s = 0.0f;
  for (int k = 0; k < nblk; ++k) s += p[(size_t)k * (DP + 1)];
  if (q < D) {
    const float tq = theta[b * (D + 1) + q];
    s = tq != 0.0f ? s * theta[b * (D + 1) + D] / tq : 0.0f;
  }
  g_theta[b * (D + 1) + q] = s;
}

// Gradient of the points x1: grid (row blocks, B, js), the sweep of k_kernel_bil with the accumulation
//   g[b, i, k] = theta_D theta_k sum_j W_ij h(r_ij) s_k,  s = theta o (x1_i - x2_j)
// A thread owns row i: nothing is reduced across threads.  `out` is g_x1 [B, M, D] when gridDim.z == 1, else the
// partials [js, B, M, D] of the column splits (the scale is applied here; k_kernel_mv_reduce only adds).
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kernel_pgrad(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const float* __restrict__ theta, int M, int N, int D,
                                                           const float* __restrict__ U, const float* __restrict__ V,
                                                           int t, float* __restrict__ out, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ float th[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
    acc[k] = 0.0f;
  }
  const float os2 = theta[b * (D + 1) + D];
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * kKoTS; e += kThreads) {
        const int j = e / kKoTS, ss = e - j * kKoTS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      float tacc[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float sd[DP];
        float r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          sd[k] = a[k] - xs[j * DP + k];
          r2 = fmaf(sd[k], sd[k], r2);
        }
        float g, h;
        kf_gh<FAMILY>(r2, &g, &h);
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
        const float wh = w * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh, sd[k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
    }
  }
  if (live) {
    float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = os2 * th[k] * acc[k];
  }
}

int ko_reduce_splits(const char* prof_name, const float* part, int js, size_t per_member, size_t total, int c,
                     const float* d, int dmode, const float* v, float* y, const int* stop, hipStream_t st) {
  LO_PROF_BEGIN(prof_name, st);
  hipLaunchKernelGGL(k_kernel_mv_reduce, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part,
                     js, per_member, total, c, d, dmode, v, y, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int ko_bil_reduce(const float* part, int nblk, int DP, int64_t B, int64_t D, const float* theta, float* g_theta,
                  hipStream_t st) {
  hipLaunchKernelGGL(k_kernel_bil_reduce, dim3((unsigned)B), dim3(64), 0, st, part, nblk, DP, (int)D, theta, g_theta);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// the product on validated arguments; part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
int kernel_mv_run(const float* x1, const float* x2, const float* theta, int64_t tstride, int family, int64_t B, int64_t M,
                  int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                  const int* stop, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_kernel_mv", st);
  ko_dispatch(family, w.DP, ko_cols{}, ko_col_chunk(c), [&](auto F, auto P, auto C) {
    hipLaunchKernelGGL((k_kernel_mv<F(), P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)tstride, (int)M,
                       (int)N, (int)D, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_kernel_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

int kernel_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1 || !ko_family_ok(op->n2)) return LO_ERR_BADARG;
  return op->R > LO_KERNEL_MAX_DIM ? LO_ERR_UNSUPPORTED : LO_OK;
}

int kernel_op_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_desc_check(&op)) return rc;
  // the launch limits of the product's kernels (batch, rows, columns): the pivoted Cholesky launches none of them
  if (!ko_shape_ok(op.B, op.N, op.N, op.R) || pl->c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  pl->ko.part = ko_split_layout<float>(*ar, op.B, op.N, op.N, pl->c);
  return LO_OK;
}

int kernel_op_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return kernel_mv_run(op.A0, op.A0, op.A1, op.R + 1, (int)op.n2, op.B, op.N, op.N, op.R, v, pl->c, op.d, op.diag_mode, y,
                       pl->ko.part, stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                     int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                     void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family)) return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_mv_run(x1, x2, theta, D + 1, family, B, M, N, D, v, c, d, diag_mode, y, part, nullptr,
                       (hipStream_t)stream);
}

size_t lo_kernel_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_bil_layout<float>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kernel_bil", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_bil<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D, U, V,
                       (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return ko_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, theta, g_theta, st);
}

size_t lo_kernel_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_kernel_pgrad", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_pgrad<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D, U,
                       V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko_reduce_splits("k_kernel_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                            LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // extern "C"

