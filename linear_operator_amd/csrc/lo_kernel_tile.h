// lo_kernel_tile.h -- what the sweeps of the matrix-free kernel family share on the device (lo_kernel_op.hip,
// lo_kernel_op_f64.hip, lo_kernel_param.hip, lo_kernel_sm.hip, lo_kernel_kinds_wide.hip).  Plain inlined functions: a kernel that uses one compiles to the
// instructions it had with the text written out (profiles/r19 holds the comparison, and the helpers that did not pass it).
#pragma once
#include "lo_internal.h"
#include "lo_kernel_fn.h"

namespace lo {

// stage the tile [jt, jt + nj) of x2, scaled coordinate by coordinate by sc, as xs[j][DP] (coordinates >= D are 0)
template <int DP, class T>
__device__ __forceinline__ void ko_stage_points(const T* __restrict__ x2b, const T* __restrict__ sc, int D, int jt, int nj,
                                                T* __restrict__ xs) {
  for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
    const int j = e / DP, dd = e - j * DP;
    xs[e] = dd < D ? x2b[(size_t)(jt + j) * D + dd] * sc[dd] : T(0);
  }
}

// ---- what the kernels of the rational-quadratic / periodic kind share (lo_kernel_param.hip, lo_kernel_kinds_wide.hip,
// lo_kernel_kinds_bil_wide.hip) -----
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

constexpr float kKpPi = 3.14159265358979323846f;

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

// ---- what the kernels of the spectral mixture kind share (lo_kernel_sm.hip, lo_kernel_kinds_wide.hip,
// lo_kernel_kinds_bil_wide.hip) ----
constexpr int kKsmQ = LO_KERNEL_SM_MAX_MIX;

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

// Sum over the 256 threads in a fixed order (wave butterfly, then waves 0..3); `red` >= 4 doubles of LDS
__device__ __forceinline__ double block_sum256_d(double v, double* red) {
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// a compensated (Kahan) running sum: the one-number-per-member entries of the derivatives, N M terms of both signs
struct KoKahan {
  float s = 0.0f, c = 0.0f;
  __device__ __forceinline__ void add(float w, float x) {
    const float term = fmaf(w, x, -c);
    const float next = s + term;
    c = (next - s) - term;
    s = next;
  }
};

}  // namespace lo
