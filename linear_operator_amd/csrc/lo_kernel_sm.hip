// lo_kernel_sm.hip -- the matrix-free spectral mixture kernel:
//   K(x1, x2)_ij = sum_{q < Q} w_q E_q prod_k c_qk,  tau = x1_i - x2_j,  E_q = exp(-2 pi^2 sum_k (sigma_qk tau_k)^2),
//   c_qk = cos(2 pi mu_qk tau_k),
// LO_OP_KERNEL_SM_DIAG and the entry points lo_kernel_sm_mv_f32 / lo_kernel_sm_bilinear_f32 / lo_kernel_sm_points_grad_f32
// of lo_amd.h.  theta [B, Q, 2 D + 1] = per mixture w, the D means mu, the D scales sigma, raw values.
//
// The sweeps are those of lo_kernel_param.hip: a workgroup owns 256 rows i of one member, one per thread, the thread keeps
// its RAW point a[DP] in registers, the raw points x2_j and the rows of v stream through LDS in tiles of 128, a tile's sums
// are formed on their own and then added to the running ones, few-row shapes split the columns j over gridDim.z
// workgroups whose partials are added in ascending order.  No float atomics.  The member's theta sits in LDS (|mu| and
// sigma padded to [Q, DP], the weights [Q]) and is read uniformly.
//   per pair   tau_k = |a_k - b_k| once (differenced first: the phase p = |mu| tau carries the error p eps, not |mu x| eps;
//              the absolute value: K(x, y) and K(y, x) have equal bits), then per mixture sum_k (sigma_k tau_k)^2, one
//              exp2, and the cosines of p in revolutions after fract (ksm_cos2pi).  Padded coordinates have mu = sigma = 0
//              and tau = 0: a factor of 1.
//   derivative (k_ksm_bil) q is a launch dimension (blockIdx.x = row block * Q + q): per workgroup one partial [2 DP + 1] =
//              the sum for w, the DP sums for mu, the DP sums for sigma; k_ksm_bil_reduce adds the workgroups in ascending
//              order and applies the factors.  With s_k = sin(2 pi mu_k tau_k):
//                d/dw = E prod c      d/dsigma_k = -4 pi^2 sigma_k tau_k^2 w E prod c
//                d/dmu_k = -2 pi tau_k s_k w E prod_{l != k} c_l
//              prod_{l != k} by a prefix and a suffix product: NO division by a cosine (a pair with mu tau = 1/4 has c = 0)
//   points     (k_ksm_pgrad) d k / d x1_k = sum_q w_q E_q sign(tau_k) (-4 pi^2 sigma_qk^2 |tau_k| prod c
//              - 2 pi |mu_qk| s_k(|.|) prod_{l != k} c_l)
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

constexpr int kKsmQ = LO_KERNEL_SM_MAX_MIX;

inline bool ksm_args_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  return ko_args_ok(B, M, N, D, c) && Q >= 1;
}
inline bool ksm_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  return D <= LO_KERNEL_SM_MAX_DIM && Q <= LO_KERNEL_SM_MAX_MIX && ko_shape_ok(B, M, N, D) && c <= 0x7fffffff;
}
using ksm_dims = std::integer_sequence<int, 4, 8, 16>;  // ko_padded_dim up to LO_KERNEL_SM_MAX_DIM

// the one layout of the derivative's workspace: a partial [2 DP + 1] per workgroup, [B, Q, rb js, 2 DP + 1]
inline float* ksm_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * Q * s.rb * s.js * (2 * ko_padded_dim(D) + 1));
}

// the member's theta in LDS: tw[q] = w_q, tmu[q][k] = |mu_qk|, tsg[q][k] = sigma_qk, both 0 for k >= D (Q DP <= 256 words)
template <int DP>
__device__ __forceinline__ void ksm_load_theta(const float* __restrict__ tb, int D, int Q, float* tw, float* tmu,
                                               float* tsg) {
  const int e = threadIdx.x;
  if (e < Q * DP) {
    const int q = e / DP, k = e - q * DP;
    const float* t = tb + q * (2 * D + 1);
    tmu[e] = k < D ? fabsf(t[1 + k]) : 0.0f;
    tsg[e] = k < D ? t[1 + D + k] : 0.0f;
  }
  if (e < Q) tw[e] = tb[e * (2 * D + 1)];
  __syncthreads();
}

// stage the tile [jt, jt + nj) of x2 as xs[j][DP], raw (coordinates >= D are 0)
template <int DP>
__device__ __forceinline__ void ksm_stage_points(const float* __restrict__ x2b, int D, int jt, int nj,
                                                 float* __restrict__ xs) {
  for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
    const int j = e / DP, dd = e - j * DP;
    xs[e] = dd < D ? x2b[(size_t)(jt + j) * D + dd] : 0.0f;
  }
}

// stage the rows [jt, jt + nj) of the right operand, columns [c0, c0 + CC) of its c, as vs[j][CC] (columns >= c are 0)
template <int CC>
__device__ __forceinline__ void ksm_stage_cols(const float* __restrict__ vb, int c, int c0, int jt, int nj,
                                               float* __restrict__ vs) {
  for (int e = threadIdx.x; e < nj * CC; e += kThreads) {
    const int j = e / CC, cc = e - j * CC;
    vs[e] = c0 + cc < c ? vb[(size_t)(jt + j) * c + c0 + cc] : 0.0f;
  }
}

// one mixture of one pair: the envelope E, the cosines c[k] and, with SINES, the sines s[k] of 2 pi |mu_k| tau_k
template <int DP, bool SINES>
__device__ __forceinline__ float ksm_mixture(const float (&tau)[DP], const float* __restrict__ mu,
                                             const float* __restrict__ sg, float (&c)[DP], float (&s)[DP]) {
  float s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float st = sg[k] * tau[k];
    s2 = fmaf(st, st, s2);
    const float p = mu[k] * tau[k];
    c[k] = ksm_cos2pi(p);
    if constexpr (SINES) s[k] = kp_sin2pi(p);
  }
  return ksm_env(s2);
}

// ex[k] = prod_{l != k} c_l by a prefix and a suffix product; returns prod_l c_l
template <int DP>
__device__ __forceinline__ float ksm_leave_one_out(const float (&c)[DP], float (&ex)[DP]) {
  float pre = 1.0f;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    ex[k] = pre;
    pre *= c[k];
  }
  float suf = 1.0f;
#pragma unroll
  for (int k = DP - 1; k >= 0; --k) {
    ex[k] *= suf;
    suf *= c[k];
  }
  return pre;
}

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c]
template <int DP, int CC>
__global__ __launch_bounds__(kThreads) void k_ksm_mv(const float* __restrict__ x1, const float* __restrict__ x2,
                                                     const float* __restrict__ theta, int Q, int M, int N, int D,
                                                     const float* __restrict__ v, int c,
                                                     const float* __restrict__ dd_ptr, int dd_mode,
                                                     float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                     const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * CC];
  __shared__ __align__(16) float tmu[kKsmQ * DP], tsg[kKsmQ * DP];
  __shared__ float tw[kKsmQ];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  ksm_load_theta<DP>(theta + b * Q * (2 * D + 1), D, Q, tw, tmu, tsg);
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
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
      ksm_stage_points<DP>(x2b, D, jt, nj, xs);
      ksm_stage_cols<CC>(vb, c, c0, jt, nj, vs);
      __syncthreads();
      float tacc[CC];
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) tacc[cc] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float tau[DP];
#pragma unroll
        for (int k = 0; k < DP; ++k) tau[k] = fabsf(a[k] - xs[j * DP + k]);
        float kv = 0.0f;
        for (int q = 0; q < Q; ++q) {
          float s2 = 0.0f, pr = 1.0f;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            const float st = tsg[q * DP + k] * tau[k];
            s2 = fmaf(st, st, s2);
            pr *= ksm_cos2pi(tmu[q * DP + k] * tau[k]);
          }
          kv = fmaf(tw[q], ksm_env(s2) * pr, kv);
        }
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
          float r = acc[cc];
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

// grid (row blocks * Q, B, js): blockIdx.x = row block * Q + q; part [B, Q, nblk = row blocks * gridDim.z, 2 DP + 1] with
// slot 0 the sum for w, 1 + k for mu_k, 1 + DP + k for sigma_k (all without their factors: k_ksm_bil_reduce)
template <int DP>
__global__ __launch_bounds__(kThreads) void k_ksm_bil(const float* __restrict__ x1, const float* __restrict__ x2,
                                                      const float* __restrict__ theta, int Q, int M, int N, int D,
                                                      const float* __restrict__ U, const float* __restrict__ V, int t,
                                                      float* __restrict__ part, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ __align__(16) float mu[DP], sg[DP];
  __shared__ float red[4];
  const int64_t b = blockIdx.y;
  const int rblk = blockIdx.x / Q, q = blockIdx.x - rblk * Q, nrb = gridDim.x / Q;
  const int i = rblk * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) {
    const int k = threadIdx.x;
    const float* tq = theta + ((size_t)b * Q + q) * (2 * D + 1);
    mu[k] = k < D ? fabsf(tq[1 + k]) : 0.0f;
    sg[k] = k < D ? tq[1 + D + k] : 0.0f;
  }
  __syncthreads();
  float a[DP], gmu[DP], gsg[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
    gmu[k] = 0.0f;
    gsg[k] = 0.0f;
  }
  KoKahan gw;
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
      ksm_stage_points<DP>(x2b, D, jt, nj, xs);
      ksm_stage_cols<kKoTS>(Vb, t, s0, jt, nj, vs);
      __syncthreads();
      float tmu[DP], tsg[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        tmu[k] = 0.0f;
        tsg[k] = 0.0f;
      }
      for (int j = 0; j < nj; ++j) {
        float tau[DP], c[DP], s[DP], ex[DP];
#pragma unroll
        for (int k = 0; k < DP; ++k) tau[k] = fabsf(a[k] - xs[j * DP + k]);
        const float E = ksm_mixture<DP, true>(tau, mu, sg, c, s);
        const float pr = ksm_leave_one_out<DP>(c, ex);
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
        const float wE = w * E;
        gw.add(wE, pr);
        const float wEp = wE * pr;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          tsg[k] = fmaf(wEp, tau[k] * tau[k], tsg[k]);
          tmu[k] = fmaf(wE * (tau[k] * s[k]), ex[k], tmu[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        gmu[k] += tmu[k];
        gsg[k] += tsg[k];
      }
    }
  }
  const size_t blk = (size_t)blockIdx.z * nrb + rblk, nblk = (size_t)nrb * gridDim.z;
  float* out = part + (((size_t)b * Q + q) * nblk + blk) * (2 * DP + 1);
  {
    const float sum = block_sum256(gw.s, red);
    if (threadIdx.x == 0) out[0] = sum;
  }
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gmu[k], red);
    if (threadIdx.x == 0) out[1 + k] = sum;
  }
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gsg[k], red);
    if (threadIdx.x == 0) out[1 + DP + k] = sum;
  }
}

// g_theta[b, q, e], e < 2 D + 1, from the nblk partials of (b, q) in ascending order.  With S the sum of the slot:
//   e == 0 (w):  S      e = 1 + k (mu_k):  -2 pi sign(mu_k) w S      e = 1 + D + k (sigma_k):  -4 pi^2 sigma_k w S
// grid (B Q), 64 threads
__global__ __launch_bounds__(64) void k_ksm_bil_reduce(const float* __restrict__ part, int nblk, int DP, int D,
                                                       const float* __restrict__ theta, float* __restrict__ g_theta) {
  const int64_t bq = blockIdx.x;
  const int e = threadIdx.x, W = 2 * DP + 1;
  if (e >= 2 * D + 1) return;
  const float* tq = theta + bq * (2 * D + 1);
  const int slot = e == 0 ? 0 : (e <= D ? e : 1 + DP + (e - 1 - D));
  const float* p = part + (size_t)bq * nblk * W + slot;
  float s = 0.0f;
  for (int k = 0; k < nblk; ++k) s += p[(size_t)k * W];
  if (e > D) s = (-4.0f * kKsmPi * kKsmPi) * tq[e] * tq[0] * s;
  else if (e > 0) s = copysignf(2.0f * kKsmPi, -tq[e]) * tq[0] * s;
  g_theta[bq * (2 * D + 1) + e] = s;
}

// Gradient of the points x1: grid (row blocks, B, js); a thread owns row i, nothing is reduced across threads.  `out` is
// g_x1 [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D] of the column splits (the scale is applied here; the
// reduction only adds).
template <int DP>
__global__ __launch_bounds__(kThreads) void k_ksm_pgrad(const float* __restrict__ x1, const float* __restrict__ x2,
                                                        const float* __restrict__ theta, int Q, int M, int N, int D,
                                                        const float* __restrict__ U, const float* __restrict__ V, int t,
                                                        float* __restrict__ out, int jchunk) {
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKoTS];
  __shared__ __align__(16) float tmu[kKsmQ * DP], tsg[kKsmQ * DP];
  __shared__ float tw[kKsmQ];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  ksm_load_theta<DP>(theta + b * Q * (2 * D + 1), D, Q, tw, tmu, tsg);
  float a[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
    acc[k] = 0.0f;
  }
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
      ksm_stage_points<DP>(x2b, D, jt, nj, xs);
      ksm_stage_cols<kKoTS>(Vb, t, s0, jt, nj, vs);
      __syncthreads();
      float tacc[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float df[DP], tau[DP], pq[DP];
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          df[k] = a[k] - xs[j * DP + k];
          tau[k] = fabsf(df[k]);
          pq[k] = 0.0f;
        }
        // pq[k] = sum_q w_q E_q (2 pi sigma_qk^2 tau_k prod c + |mu_qk| s_k prod_{l != k} c_l); the factor -2 pi at the end
        for (int q = 0; q < Q; ++q) {
          float c[DP], s[DP], ex[DP];
          const float* mu = tmu + q * DP;
          const float* sg = tsg + q * DP;
          const float E = ksm_mixture<DP, true>(tau, mu, sg, c, s);
          const float pr = ksm_leave_one_out<DP>(c, ex);
          const float wE = tw[q] * E;
          const float wEp = (2.0f * kKsmPi) * wE * pr;
#pragma unroll
          for (int k = 0; k < DP; ++k)
            pq[k] = fmaf(wEp * (sg[k] * sg[k]), tau[k], fmaf(wE * (mu[k] * s[k]), ex[k], pq[k]));
        }
        float w = 0.0f;
#pragma unroll
        for (int ss = 0; ss < kKoTS; ++ss) w = fmaf(u[ss], vs[j * kKoTS + ss], w);
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fmaf(df[k] < 0.0f ? -w : w, pq[k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
    }
  }
  if (live) {
    float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = (-2.0f * kKsmPi) * acc[k];
  }
}

// the product on validated arguments; part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
static int kernel_sm_mv_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                            int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                            const int* stop, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_ksm_mv", st);
  ko_pick(ksm_dims{}, w.DP, [&](auto P) {
    ko_pick(ko_cols{}, ko_col_chunk(c), [&](auto C) {
      hipLaunchKernelGGL((k_ksm_mv<P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, Q, (int)M, (int)N, (int)D, v,
                         (int)c, d, dmode, y, p, w.s.jchunk, stop);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_ksm_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y, stop,
                            st);
  return LO_OK;
}

int kernel_sm_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1 || op->n2 < 1) return LO_ERR_BADARG;
  return (op->R > LO_KERNEL_SM_MAX_DIM || op->n2 > LO_KERNEL_SM_MAX_MIX) ? LO_ERR_UNSUPPORTED : LO_OK;
}

int kernel_sm_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_sm_desc_check(&op)) return rc;
  // the launch limits of the product's kernels (batch, rows, columns): the pivoted Cholesky launches none of them
  if (!ksm_shape_ok(op.B, op.N, op.N, op.R, op.n2, pl->c)) return LO_ERR_UNSUPPORTED;
  pl->ko.part = ko_split_layout<float>(*ar, op.B, op.N, op.N, pl->c);
  return LO_OK;
}

int kernel_sm_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return kernel_sm_mv_run(op.A0, op.A0, op.A1, (int)op.n2, op.B, op.N, op.N, op.R, v, pl->c, op.d, op.diag_mode, y,
                          pl->ko.part, stop, st);
}

// the entry points' diagonal operand: ko_diag_ok, and no mode at all on a rectangular product
static bool ksm_diag_ok(int diag_mode, const void* d, bool square) {
  return ko_diag_ok(diag_mode, d, square) && (square || diag_mode == LO_DIAG_NONE);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_sm_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  if (!ksm_args_ok(B, M, N, D, Q, c) || !ksm_shape_ok(B, M, N, D, Q, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_sm_mv_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M, int64_t N,
                        int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ksm_args_ok(B, M, N, D, Q, c)) return LO_ERR_BADARG;
  if (!ksm_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_sm_mv_run(x1, x2, theta, Q, B, M, N, D, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

size_t lo_kernel_sm_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t) {
  if (!ksm_args_ok(B, M, N, D, Q, t) || !ksm_shape_ok(B, M, N, D, Q, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ksm_bil_layout(ar, B, M, N, D, Q); });
}

int lo_kernel_sm_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                              size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ksm_args_ok(B, M, N, D, Q, t)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ksm_bil_layout(ar, B, M, N, D, Q);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  const dim3 grid((unsigned)(w.s.rb * Q), (unsigned)B, (unsigned)w.s.js);  // (rb <= 2^23, Q <= 16)
  LO_PROF_BEGIN("k_ksm_bil", st);
  ko_pick(ksm_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_ksm_bil<P()>), grid, dim3(kThreads), 0, st, x1, x2, theta, (int)Q, (int)M, (int)N, (int)D, U, V,
                       (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ksm_bil_reduce, dim3((unsigned)(B * Q)), dim3(64), 0, st, part, w.s.rb * w.s.js, w.DP, (int)D, theta,
                     g_theta);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

size_t lo_kernel_sm_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t) {
  if (!ksm_args_ok(B, M, N, D, Q, t) || !ksm_shape_ok(B, M, N, D, Q, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_sm_points_grad_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                                 int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ksm_args_ok(B, M, N, D, Q, t)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_ksm_pgrad", st);
  ko_pick(ksm_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_ksm_pgrad<P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)Q, (int)M, (int)N, (int)D, U,
                       V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko_reduce_splits("k_ksm_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                            LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // extern "C"
