// lo_kernel_param.hip -- the matrix-free kernels with a shape parameter, rational quadratic and periodic:
// K(x1, x2)_ij = os2 g(x1_i, x2_j), LO_OP_KERNEL_PARAM_DIAG and the entry points lo_kernel_param_mv_f32 /
// lo_kernel_param_bilinear_f32 / lo_kernel_param_points_grad_f32 of lo_amd.h.  theta [B, 2 D + 2] = the D inverse
// lengthscales t, os2, alpha, the D inverse periods nu (one layout for both families).
//
// The sweeps are those of lo_kernel_op.hip: a workgroup owns 256 rows i of one member, one per thread, the thread keeps its
// scaled point a[DP] in registers, the points x2_j (scaled the same way while they are staged) and the rows of v stream
// through LDS in tiles of 128, a tile's sums are formed on their own and then added to the running ones, few-row shapes
// split the columns j over gridDim.z workgroups whose partials are added in ascending order.  No float atomics.
//   RQ        a = t o x1_i, the tile holds t o x2_j: r^2 by direct differences as for RBF, q = r^2 / (2 alpha),
//             g = exp2(-alpha log2(1 + q)), h = -g / (1 + q), dg/dalpha = g (q / (1 + q) - ln(1 + q)) (kp_rq_gha)
//   PERIODIC  a = nu o x1_i, the tile holds nu o x2_j: phi_k = a_k - b_k, s_k = sin(pi |phi_k|), rho = sum_k (t_k s_k)^2,
//             g = exp(-2 rho);  t_k dg/dt_k = -4 g (t_k s_k)^2,  nu_k dg/dnu_k = -2 pi g t_k^2 phi_k sin(2 pi phi_k),
//             dg/dx1_k = -2 pi g t_k^2 nu_k sin(2 pi phi_k).  Padded coordinates have t_k = nu_k = 0: they add nothing.
// Derivative (k_kparam_bil): per workgroup one partial [2 DP + 2] = the DP lengthscale sums, the os2 sum, the alpha sum,
//   the DP period sums, by fixed-order block sums; k_kparam_bil_reduce adds the workgroups in ascending order, applies the
//   factors and writes 0 into the entries the family does not read.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

constexpr float kKpPi = 3.14159265358979323846f;

inline bool kp_family_ok(int64_t family) { return family == LO_KERNEL_RQ || family == LO_KERNEL_PERIODIC; }
inline bool kp_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D) {
  return D <= LO_KERNEL_PARAM_MAX_DIM && ko_shape_ok(B, M, N, D);
}
using kp_families = std::integer_sequence<int, LO_KERNEL_RQ, LO_KERNEL_PERIODIC>;
template <class F>
inline void kp_dispatch(int family, int DP, F&& f) {
  ko_pick(kp_families{}, family, [&](auto fam) { ko_pick(ko_dims{}, DP, [&](auto dp) { f(fam, dp); }); });
}

// the one layout of the derivative's workspace: a partial [2 DP + 2] per workgroup, [B, rb js, 2 DP + 2]
inline float* kp_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * s.rb * s.js * (2 * ko_padded_dim(D) + 2));
}

// what a workgroup reads of its member's theta: th[k] = t_k, sc[k] = the factor the points are scaled by (RQ: t_k,
// PERIODIC: nu_k), both 0 for k >= D
template <int FAMILY, int DP>
__device__ __forceinline__ void kp_load_theta(const float* __restrict__ tb, int D, float* th, float* sc) {
  if (threadIdx.x < DP) {
    const int k = threadIdx.x;
    const float t = k < D ? tb[k] : 0.0f;
    th[k] = t;
    sc[k] = FAMILY == LO_KERNEL_PERIODIC ? (k < D ? tb[D + 2 + k] : 0.0f) : t;
  }
  __syncthreads();
}

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c]
template <int FAMILY, int DP, int CC>
__global__ __launch_bounds__(kThreads) void k_kparam_mv(const float* __restrict__ x1, const float* __restrict__ x2,
                                                        const float* __restrict__ theta, int M, int N, int D,
                                                        const float* __restrict__ v, int c,
                                                        const float* __restrict__ dd_ptr, int dd_mode,
                                                        float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                        const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * CC];
  __shared__ float th[DP], sc[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const float* tb = theta + b * (2 * D + 2);
  kp_load_theta<FAMILY, DP>(tb, D, th, sc);
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * sc[k] : 0.0f;
  const float os2 = tb[D], alpha = tb[D + 1];
  const float inv2a = 0.5f / alpha;  // (RQ only; PERIODIC never reads it)
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
      ko_stage_points<DP>(x2b, sc, D, jt, nj, xs);
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
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float df = a[k] - xs[j * DP + k];
          if constexpr (FAMILY == LO_KERNEL_PERIODIC) {
            const float ts = th[k] * kp_sinpi(fabsf(df));
            sum = fmaf(ts, ts, sum);
          } else {
            sum = fmaf(df, df, sum);
          }
        }
        const float kv = FAMILY == LO_KERNEL_PERIODIC ? kp_per_g(sum) : kp_rq_g(sum, alpha, inv2a);
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

// The pair of the two derivative sweeps: from the thread's point a and the tile's point xs[j] the value g and per
// coordinate what the lengthscale / period / points sums take.
//   RQ:        g, h, ga as kp_rq_gha; e1[k] = the scaled difference s_k (lengthscale: h s_k^2, points: h s_k)
//   PERIODIC:  g; e1[k] = (t_k s_k)^2, e2[k] = t_k^2 |phi_k| sin(2 pi |phi_k|) (even in phi), or with POINTS
//              e2[k] = sin(2 pi phi_k) (odd: the sign put back)
template <int FAMILY, int DP, bool POINTS>
__device__ __forceinline__ void kp_pair(const float (&a)[DP], const float* __restrict__ xj, const float* __restrict__ th,
                                        float alpha, float inv2a, float* g, float* h, float* ga, float (&e1)[DP],
                                        float (&e2)[DP]) {
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float df = a[k] - xj[k];
    if constexpr (FAMILY == LO_KERNEL_PERIODIC) {
      const float p = fabsf(df);
      const float ts = th[k] * kp_sinpi(p);
      const float s2 = kp_sin2pi(p);
      e1[k] = ts * ts;
      e2[k] = POINTS ? (df < 0.0f ? -s2 : s2) : th[k] * th[k] * p * s2;
      sum += e1[k];
    } else {
      e1[k] = df;
      sum = fmaf(df, df, sum);
    }
  }
  if constexpr (FAMILY == LO_KERNEL_PERIODIC) {
    *g = kp_per_g(sum);
    *h = 0.0f;
    *ga = 0.0f;
  } else {
    kp_rq_gha(sum, alpha, inv2a, g, h, ga);
  }
}

// grid (row blocks, B, js); part [B, nblk = gridDim.x * gridDim.z, 2 DP + 2]
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kparam_bil(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ theta, int M, int N, int D,
                                                         const float* __restrict__ U, const float* __restrict__ V, int t,
                                                         float* __restrict__ part, int jchunk) {
  constexpr bool PER = FAMILY == LO_KERNEL_PERIODIC;
  constexpr int DQ = PER ? DP : 1;  // the period sums exist for PERIODIC only
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ float th[DP], sc[DP];
  __shared__ float red[4];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const float* tb = theta + b * (2 * D + 2);
  kp_load_theta<FAMILY, DP>(tb, D, th, sc);
  float a[DP], gacc[DP], pacc[DQ];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * sc[k] : 0.0f;
    gacc[k] = 0.0f;
  }
#pragma unroll
  for (int k = 0; k < DQ; ++k) pacc[k] = 0.0f;
  const float alpha = tb[D + 1];
  const float inv2a = 0.5f / alpha;
  KoKahan gos, gal;
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
      ko_stage_points<DP>(x2b, sc, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * kKoTS; e += kThreads) {
        const int j = e / kKoTS, ss = e - j * kKoTS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      float tacc[DP], tpacc[DQ];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < DQ; ++k) tpacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float e1[DP], e2[DP];
        float g, h, ga;
        kp_pair<FAMILY, DP, false>(a, xs + j * DP, th, alpha, inv2a, &g, &h, &ga, e1, e2);
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
        gos.add(w, g);
        if constexpr (PER) {
          const float wg = w * g;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            tacc[k] = fmaf(wg, e1[k], tacc[k]);
            tpacc[k] = fmaf(wg, e2[k], tpacc[k]);
          }
        } else {
          gal.add(w, ga);
          const float wh = w * h;
#pragma unroll
          for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh * e1[k], e1[k], tacc[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
      if constexpr (PER) {
#pragma unroll
        for (int k = 0; k < DP; ++k) pacc[k] += tpacc[k];
      }
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
  float* out = part + ((size_t)b * nblk + blk) * (2 * DP + 2);
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gacc[k], red);
    if (threadIdx.x == 0) out[k] = sum;
  }
  {
    const float sum = block_sum256(gos.s, red);
    if (threadIdx.x == 0) out[DP] = sum;
  }
  {
    const float sum = block_sum256(gal.s, red);
    if (threadIdx.x == 0) out[DP + 1] = sum;
  }
  if constexpr (PER) {  // (RQ: the period slots are never read)
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float sum = block_sum256(pacc[k], red);
      if (threadIdx.x == 0) out[DP + 2 + k] = sum;
    }
  }
}

// g_theta[b, q], q < 2 D + 2, from the nblk partials in ascending order.  With S the sum of the slot:
//   q < D (t_q):     RQ os2 S / t_q          PERIODIC -4 os2 S / t_q        q == D (os2):  S
//   q == D + 1:      RQ os2 S                PERIODIC 0                     q > D + 1 (nu_k): RQ 0, PERIODIC -2 pi os2 S / nu_k
__global__ __launch_bounds__(128) void k_kparam_bil_reduce(const float* __restrict__ part, int nblk, int DP, int D,
                                                           int family, const float* __restrict__ theta,
                                                           float* __restrict__ g_theta) {
  const int64_t b = blockIdx.x;
  const int q = threadIdx.x, W = 2 * DP + 2;
  if (q >= 2 * D + 2) return;
  const bool per = family == LO_KERNEL_PERIODIC;
  const float* tb = theta + b * (2 * D + 2);
  const int slot = q < D ? q : (q <= D + 1 ? DP + (q - D) : DP + 2 + (q - D - 2));
  const bool read = q <= D || (q == D + 1 ? !per : per);
  float s = 0.0f;
  if (read) {
    const float* p = part + (size_t)b * nblk * W + slot;
    for (int k = 0; k < nblk; ++k) s += p[(size_t)k * W];
    const float os2 = tb[D];
    if (q < D) {
      s = tb[q] != 0.0f ? (per ? -4.0f : 1.0f) * s * os2 / tb[q] : 0.0f;
    } else if (q == D + 1) {
      s = s * os2;
    } else if (q > D + 1) {
      s = tb[q] != 0.0f ? (-2.0f * kKpPi) * s * os2 / tb[q] : 0.0f;
    }
  }
  g_theta[b * (2 * D + 2) + q] = s;
}

// Gradient of the points x1: grid (row blocks, B, js); a thread owns row i, nothing is reduced across threads.
//   RQ        g[b, i, k] = os2 t_k sum_j W_ij h s_k                       (s the scaled difference)
//   PERIODIC  g[b, i, k] = -2 pi os2 t_k^2 nu_k sum_j W_ij g sin(2 pi phi_k)
// `out` is g_x1 [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D] of the column splits (the scale is applied
// here; the reduction only adds).
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kparam_pgrad(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const float* __restrict__ theta, int M, int N, int D,
                                                           const float* __restrict__ U, const float* __restrict__ V,
                                                           int t, float* __restrict__ out, int jchunk) {
  constexpr bool PER = FAMILY == LO_KERNEL_PERIODIC;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ float th[DP], sc[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const float* tb = theta + b * (2 * D + 2);
  kp_load_theta<FAMILY, DP>(tb, D, th, sc);
  float a[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * sc[k] : 0.0f;
    acc[k] = 0.0f;
  }
  const float os2 = tb[D], alpha = tb[D + 1];
  const float inv2a = 0.5f / alpha;
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
      ko_stage_points<DP>(x2b, sc, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * kKoTS; e += kThreads) {
        const int j = e / kKoTS, ss = e - j * kKoTS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      float tacc[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float e1[DP], e2[DP];
        float g, h, ga;
        kp_pair<FAMILY, DP, true>(a, xs + j * DP, th, alpha, inv2a, &g, &h, &ga, e1, e2);
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
        const float wf = w * (PER ? g : h);
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wf, PER ? e2[k] : e1[k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
    }
  }
  if (live) {
    float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = PER ? (-2.0f * kKpPi) * os2 * th[k] * th[k] * sc[k] * acc[k] : os2 * th[k] * acc[k];
  }
}

// the product on validated arguments; part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
static int kernel_param_mv_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                               int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y,
                               float* part, const int* stop, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_kparam_mv", st);
  kp_dispatch(family, w.DP, [&](auto F, auto P) {
    ko_pick(ko_cols{}, ko_col_chunk(c), [&](auto C) {
      hipLaunchKernelGGL((k_kparam_mv<F(), P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D,
                         v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_kparam_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

int kernel_param_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1 || !kp_family_ok(op->n2)) return LO_ERR_BADARG;
  return op->R > LO_KERNEL_PARAM_MAX_DIM ? LO_ERR_UNSUPPORTED : LO_OK;
}

int kernel_param_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_param_desc_check(&op)) return rc;
  // the launch limits of the product's kernels (batch, rows, columns): the pivoted Cholesky launches none of them
  if (!kp_shape_ok(op.B, op.N, op.N, op.R) || pl->c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  pl->ko.part = ko_split_layout<float>(*ar, op.B, op.N, op.N, pl->c);
  return LO_OK;
}

int kernel_param_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return kernel_param_mv_run(op.A0, op.A0, op.A1, (int)op.n2, op.B, op.N, op.N, op.R, v, pl->c, op.d, op.diag_mode, y,
                             pl->ko.part, stop, st);
}

// the entry points' diagonal operand: ko_diag_ok, and no mode at all on a rectangular product
static bool kp_diag_ok(int diag_mode, const void* d, bool square) {
  return ko_diag_ok(diag_mode, d, square) && (square || diag_mode == LO_DIAG_NONE);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_param_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !kp_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_param_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                           void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c) || !kp_family_ok(family)) return LO_ERR_BADARG;
  if (!kp_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_param_mv_run(x1, x2, theta, family, B, M, N, D, v, c, d, diag_mode, y, part, nullptr,
                             (hipStream_t)stream);
}

size_t lo_kernel_param_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { kp_bil_layout(ar, B, M, N, D); });
}

int lo_kernel_param_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                 int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                 float* g_theta, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !kp_family_ok(family))
    return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = kp_bil_layout(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kparam_bil", st);
  kp_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kparam_bil<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D, U, V,
                       (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kparam_bil_reduce, dim3((unsigned)B), dim3(128), 0, st, part, w.s.rb * w.s.js, w.DP, (int)D,
                     (int)family, theta, g_theta);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

size_t lo_kernel_param_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_param_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                    int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                    float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !kp_family_ok(family))
    return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_kparam_pgrad", st);
  kp_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kparam_pgrad<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D, U,
                       V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko_reduce_splits("k_kparam_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                            LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // extern "C"
