// lo_kernel_task.hip -- the matrix-free task-indexed ("Hadamard") multitask operator
//   K(x1, x2)_ij = os2 g(|(x1_i - x2_j) / l|) Bt[t_i, t_j],
// LO_OP_KERNEL_TASK_DIAG and the entry points lo_kernel_task_mv_f32 / lo_kernel_task_bilinear_f32 /
// lo_kernel_task_points_grad_f32 of lo_amd.h.  A point is a row of D coordinates and then the task id of the observation,
// an integer 0 .. T - 1 stored as a float (the covar_func of such an operator gathers an index kernel at the ids and
// multiplies the data kernel by it, densely; here K is never in memory and the tasks need not share their points).
//
// The three kernels are the pair sweep of lo_kernel_op.hip: a workgroup owns 256 rows i of one member, one per thread,
// the thread's point scaled once into DP registers; x2, scaled the same way while it is staged, streams through LDS in
// tiles of 128 and every lane reads the same tile entry (broadcast); r^2 by direct differences; a tile's sums formed on
// their own and then added to the running ones; few rows: the columns j split as in ko_shape, the partials added in
// ascending order by k_kernel_mv_reduce.  Ragged M, N, D, c are predicated.  What is new:
//   * the tile also stages the task ids, converted once (tk_task_id: round to nearest, clamp into [0, T - 1]) and stored
//     as t_j T, so that a pair's table address is one add: bt[t_j T + t_i];
//   * Bt (<= 64 floats) sits in LDS TRANSPOSED.  t_j is the same for all lanes of a wave, t_i is the lane's own: the lanes
//     touch at most T consecutive words, a read without bank conflicts.  No per-thread array is indexed at run time.
// Derivative (k_kernel_task_bil): a thread's row has ONE task a = t_i, so the thread accumulates S[b] += W_ij g for the T
//   values b of t_j (8 registers, chosen by an unrolled compare / select) and the lengthscale sums with W_ij Bt[t_i, t_j] h.
//   Each S[a, b] is one number per member, a sum of about M N / T^2 terms of both signs, as the outputscale sum of
//   k_kernel_bil is; compensating all 8 accumulators per pair would triple the pair's cost, so S is summed plainly over
//   sub-tiles of 8 pairs and every join above that is compensated (Kahan): the sub-tile into the thread's running sum, the
//   256 rows into the workgroup's partial [T, T] (through LDS, entry (a, b): the rows with t_i = a in ascending order), the
//   workgroups' partials in k_kernel_task_bil_reduce.  The lengthscale sums are two-level and go through fixed-order
//   block sums, as in k_kernel_bil.  The reduce writes g_task = os2 S, the outputscale entry sum_ab Bt[a, b] S[a, b] and
//   the lengthscale entries as k_kernel_bil_reduce does.  No float atomics: two calls give equal bits; a task without a
//   point gets exact zeros.
// Points (k_kernel_task_pgrad): the sweep of k_kernel_pgrad with W_ij Bt[t_i, t_j] h; the task column of g_x1 is written 0.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_task.h"

namespace lo {

constexpr int kTkMaxT = LO_KERNEL_TASK_MAX_TASKS;

inline bool tk_tasks_ok(int64_t T) { return T >= 1 && T <= LO_KERNEL_TASK_MAX_TASKS; }
// D coordinates and the id column are one point of D + 1 floats
inline bool tk_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D) { return ko_shape_ok(B, M, N, D + 1); }

constexpr int kTkSub = 8;  // pairs per sub-tile of the derivative's S sums

// *s += term with the running compensation *c (Kahan): the sums S[a, b] are long sums of both signs
__device__ __forceinline__ void kahan_add(float term, float* __restrict__ s, float* __restrict__ c) {
  const float t = term - *c;
  const float next = *s + t;
  *c = (next - *s) - t;
  *s = next;
}

// stage the tile [jt, jt + nj) of x2 (rows of D + 1 floats): the coordinates scaled by the inverse lengthscales as
// xs[j][DP] (coordinates >= D are 0), the task ids as tsT[j] = t_j T
template <int DP>
__device__ __forceinline__ void tk_stage_points(const float* __restrict__ x2b, const float* __restrict__ th, int D, int T,
                                                int jt, int nj, float* __restrict__ xs, int* __restrict__ tsT) {
  const int DX = D + 1;
  for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
    const int j = e / DP, dd = e - j * DP;
    xs[e] = dd < D ? x2b[(size_t)(jt + j) * DX + dd] * th[dd] : 0.0f;
  }
  for (int j = threadIdx.x; j < nj; j += kThreads) tsT[j] = tk_task_id(x2b[(size_t)(jt + j) * DX + D], T) * T;
}

// theta's inverse lengthscales into th[DP] and Bt of member b TRANSPOSED into bt: bt[t_j T + t_i] = Bt[t_i, t_j]
template <int DP>
__device__ __forceinline__ void tk_stage_params(const float* __restrict__ theta, const float* __restrict__ task, int64_t b,
                                                int D, int T, float* __restrict__ th, float* __restrict__ bt) {
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0f;
  if ((int)threadIdx.x < T * T) {
    const int ti = threadIdx.x / T, tj = threadIdx.x - ti * T;
    bt[tj * T + ti] = task[b * T * T + threadIdx.x];
  }
}

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c]
template <int FAMILY, int DP, int CC>
__global__ __launch_bounds__(kThreads) void k_kernel_task_mv(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             const float* __restrict__ theta,
                                                             const float* __restrict__ task, int M, int N, int D, int T,
                                                             const float* __restrict__ v, int c,
                                                             const float* __restrict__ dd_ptr, int dd_mode,
                                                             float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                             const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * CC];
  __shared__ int tsT[kKoTJ];
  __shared__ float th[DP];
  __shared__ float bt[kTkMaxT * kTkMaxT];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const int DX = D + 1;
  tk_stage_params<DP>(theta, task, b, D, T, th, bt);
  __syncthreads();
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * DX + k] * th[k] : 0.0f;
  const int ti = live ? tk_task_id(x1[((size_t)b * M + i) * DX + D], T) : 0;
  const float os2 = theta[b * DX + D];
  const float* x2b = x2 + (size_t)b * N * DX;
  const float* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += CC) {
    float acc[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      tk_stage_points<DP>(x2b, th, D, T, jt, nj, xs, tsT);
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
        const float kv = kf_g<FAMILY>(r2) * bt[tsT[j] + ti];
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

// grid (row blocks, B, js); part [B, nblk = gridDim.x * gridDim.z, DP + T T]: the DP lengthscale sums, then S [T, T]
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kernel_task_bil(const float* __restrict__ x1, const float* __restrict__ x2,
                                                              const float* __restrict__ theta,
                                                              const float* __restrict__ task, int M, int N, int D, int T,
                                                              const float* __restrict__ U, const float* __restrict__ V,
                                                              int t, float* __restrict__ part, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ int tsT[kKoTJ];
  __shared__ float th[DP];
  __shared__ float bt[kTkMaxT * kTkMaxT];
  __shared__ float red[4];
  __shared__ float rowS[kThreads * kTkMaxT];  // the rows' S sums and tasks, for the workgroup's partial [T, T]
  __shared__ int rowT[kThreads];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const int DX = D + 1;
  tk_stage_params<DP>(theta, task, b, D, T, th, bt);
  __syncthreads();
  float a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * DX + k] * th[k] : 0.0f;
    gacc[k] = 0.0f;
  }
  const int ti = live ? tk_task_id(x1[((size_t)b * M + i) * DX + D], T) : 0;
  float S[kTkMaxT], Sc[kTkMaxT];
#pragma unroll
  for (int bb = 0; bb < kTkMaxT; ++bb) S[bb] = Sc[bb] = 0.0f;
  const float* x2b = x2 + (size_t)b * N * DX;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();
      tk_stage_points<DP>(x2b, th, D, T, jt, nj, xs, tsT);
      for (int e = threadIdx.x; e < nj * kKoTS; e += kThreads) {
        const int j = e / kKoTS, ss = e - j * kKoTS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      float tacc[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int jb = 0; jb < nj; jb += kTkSub) {  // S: sub-tiles of kTkSub pairs, each joined by a compensated addition
        const int je = min(nj, jb + kTkSub);
        float tS[kTkMaxT];
#pragma unroll
        for (int bb = 0; bb < kTkMaxT; ++bb) tS[bb] = 0.0f;
        for (int j = jb; j < je; ++j) {
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
          const int tjT = tsT[j];
          const float wg = w * g;
#pragma unroll
          for (int bb = 0; bb < kTkMaxT; ++bb) tS[bb] += tjT == bb * T ? wg : 0.0f;
          const float wh = w * bt[tjT + ti] * h;
#pragma unroll
          for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh * sd[k], sd[k], tacc[k]);
        }
#pragma unroll
        for (int bb = 0; bb < kTkMaxT; ++bb) kahan_add(tS[bb], &S[bb], &Sc[bb]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
  float* out = part + ((size_t)b * nblk + blk) * (DP + T * T);
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gacc[k], red);
    if (threadIdx.x == 0) out[k] = sum;
  }
#pragma unroll
  for (int bb = 0; bb < kTkMaxT; ++bb) rowS[threadIdx.x * kTkMaxT + bb] = S[bb];
  rowT[threadIdx.x] = ti;
  __syncthreads();
  if ((int)threadIdx.x < T * T) {  // entry (a, bb): the rows of task a in ascending order, compensated
    const int ta = threadIdx.x / T, bb = threadIdx.x - ta * T;
    float s = 0.0f, sc = 0.0f;
#pragma unroll 4
    for (int r = 0; r < kThreads; ++r) kahan_add(rowT[r] == ta ? rowS[r * kTkMaxT + bb] : 0.0f, &s, &sc);
    out[DP + threadIdx.x] = s;
  }
}

// From the nblk partials in ascending order: g_theta[b, q < D] = os2 / theta[q] times the sum, g_task[b] = os2 S,
// g_theta[b, D] = sum_ab Bt[a, b] S[a, b] (ascending).  One workgroup of 128 per member: threads 0 .. D - 1 the
// lengthscale slots (D <= 31), threads 32 .. 32 + T T - 1 the entries of S.
__global__ __launch_bounds__(128) void k_kernel_task_bil_reduce(const float* __restrict__ part, int nblk, int DP, int D,
                                                                int T, const float* __restrict__ theta,
                                                                const float* __restrict__ task,
                                                                float* __restrict__ g_theta, float* __restrict__ g_task) {
  __shared__ float sS[kTkMaxT * kTkMaxT];
  const int64_t b = blockIdx.x;
  const int q = threadIdx.x, PS = DP + T * T;
  const float* p = part + (size_t)b * nblk * PS;
  const float os2 = theta[b * (D + 1) + D];
  if (q < D) {
    float s = 0.0f;
    for (int k = 0; k < nblk; ++k) s += p[(size_t)k * PS + q];
    const float tq = theta[b * (D + 1) + q];
    g_theta[b * (D + 1) + q] = tq != 0.0f ? s * os2 / tq : 0.0f;
  } else if (q >= 32 && q < 32 + T * T) {
    const int e = q - 32;
    float s = 0.0f, sc = 0.0f;
    for (int k = 0; k < nblk; ++k) kahan_add(p[(size_t)k * PS + DP + e], &s, &sc);
    sS[e] = s;
    g_task[b * T * T + e] = os2 * s;
  }
  __syncthreads();
  if (q == 0) {
    float s = 0.0f;
    for (int e = 0; e < T * T; ++e) s = fmaf(task[b * T * T + e], sS[e], s);
    g_theta[b * (D + 1) + D] = s;
  }
}

// Gradient of the points x1: grid (row blocks, B, js), the sweep of k_kernel_task_bil with the accumulation
//   g[b, i, k] = theta_D theta_k sum_j W_ij Bt[t_i, t_j] h(r_ij) s_k,  s = theta o (x1_i - x2_j),  g[b, i, D] = 0
// A thread owns row i: nothing is reduced across threads.  `out` is g_x1 [B, M, D + 1] when gridDim.z == 1, else the
// partials [js, B, M, D + 1] of the column splits (the scale is applied here; k_kernel_mv_reduce only adds).
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kernel_task_pgrad(const float* __restrict__ x1, const float* __restrict__ x2,
                                                                const float* __restrict__ theta,
                                                                const float* __restrict__ task, int M, int N, int D, int T,
                                                                const float* __restrict__ U, const float* __restrict__ V,
                                                                int t, float* __restrict__ out, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ int tsT[kKoTJ];
  __shared__ float th[DP];
  __shared__ float bt[kTkMaxT * kTkMaxT];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const int DX = D + 1;
  tk_stage_params<DP>(theta, task, b, D, T, th, bt);
  __syncthreads();
  float a[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * DX + k] * th[k] : 0.0f;
    acc[k] = 0.0f;
  }
  const int ti = live ? tk_task_id(x1[((size_t)b * M + i) * DX + D], T) : 0;
  const float os2 = theta[b * DX + D];
  const float* x2b = x2 + (size_t)b * N * DX;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      tk_stage_points<DP>(x2b, th, D, T, jt, nj, xs, tsT);
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
        const float wh = w * bt[tsT[j] + ti] * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh, sd[k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
    }
  }
  if (live) {
    float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * DX;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = os2 * th[k] * acc[k];
    o[D] = 0.0f;
  }
}

// the product on validated arguments; part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
static int tk_mv_run(const float* x1, const float* x2, const float* theta, const float* task, int family, int64_t B,
                     int64_t M, int64_t N, int64_t D, int64_t T, const float* v, int64_t c, const float* d, int dmode,
                     float* y, float* part, const int* stop, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_kernel_task_mv", st);
  ko_dispatch(family, w.DP, ko_cols{}, ko_col_chunk(c), [&](auto F, auto P, auto C) {
    hipLaunchKernelGGL((k_kernel_task_mv<F(), P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, task, (int)M,
                       (int)N, (int)D, (int)T, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_kernel_task_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

// the workgroups' partials [B, rb js, DP + T T] of the derivative
static float* tk_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D, int64_t T) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * s.rb * s.js * (ko_padded_dim(D) + T * T));
}

int kernel_task_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || !op->task || op->R < 1 || !ko_family_ok(op->n2) || op->nterms < 1) return LO_ERR_BADARG;
  if (op->R + 1 > LO_KERNEL_MAX_DIM || op->nterms > LO_KERNEL_TASK_MAX_TASKS) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

int kernel_task_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_task_desc_check(&op)) return rc;
  if (!tk_shape_ok(op.B, op.N, op.N, op.R) || pl->c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  pl->kt.part = ko_split_layout<float>(*ar, op.B, op.N, op.N, pl->c);
  return LO_OK;
}

int kernel_task_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return tk_mv_run(op.A0, op.A0, op.A1, op.task, (int)op.n2, op.B, op.N, op.N, op.R, op.nterms, v, pl->c, op.d,
                   op.diag_mode, y, pl->kt.part, stop, st);
}

// what every sizer and entry point asks of its sizes (`cols`: c or t)
static bool tk_sizes_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t cols) {
  return ko_args_ok(B, M, N, D, cols) && tk_tasks_ok(T) && tk_shape_ok(B, M, N, D) && cols <= 0x7fffffff;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_task_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t c) {
  if (!tk_sizes_ok(B, M, N, D, T, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_task_mv_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                          int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* v, int64_t c, const float* d,
                          int32_t diag_mode, float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !task || !v || !y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family) || T < 1)
    return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!tk_sizes_ok(B, M, N, D, T, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return tk_mv_run(x1, x2, theta, task, family, B, M, N, D, T, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

size_t lo_kernel_task_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t) {
  if (!tk_sizes_ok(B, M, N, D, T, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { tk_bil_layout(ar, B, M, N, D, T); });
}

int lo_kernel_task_bilinear_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                                int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* U, const float* V,
                                int64_t t, float* g_theta, float* g_task, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !task || !U || !V || !g_theta || !g_task || !ko_args_ok(B, M, N, D, t) ||
      !ko_family_ok(family) || T < 1)
    return LO_ERR_BADARG;
  if (!tk_sizes_ok(B, M, N, D, T, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = tk_bil_layout(ar, B, M, N, D, T);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kernel_task_bil", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_task_bil<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, task, (int)M, (int)N,
                       (int)D, (int)T, U, V, (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kernel_task_bil_reduce, dim3((unsigned)B), dim3(128), 0, st, part, w.s.rb * w.s.js, w.DP, (int)D,
                     (int)T, theta, task, g_theta, g_task);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

size_t lo_kernel_task_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t) {
  if (!tk_sizes_ok(B, M, N, D, T, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D + 1); });
}

int lo_kernel_task_points_grad_f32(const float* x1, const float* x2, const float* theta, const float* task, int32_t family,
                                   int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, const float* U, const float* V,
                                   int64_t t, float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !task || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family) || T < 1)
    return LO_ERR_BADARG;
  if (!tk_sizes_ok(B, M, N, D, T, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D + 1);  // [js, B, M, D + 1]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_kernel_task_pgrad", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_task_pgrad<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, task, (int)M, (int)N,
                       (int)D, (int)T, U, V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D + 1 as its columns and no diagonal)
    return ko_reduce_splits("k_kernel_task_pgrad_reduce", part, w.s.js, (size_t)M * (D + 1), (size_t)B * M * (D + 1),
                            (int)(D + 1), nullptr, LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // extern "C"

