// lo_kernel_tile.h -- what the sweeps of the matrix-free kernel family share on the device (lo_kernel_op.hip,
// lo_kernel_op_f64.hip, lo_kernel_param.hip, lo_kernel_sm.hip, lo_kernel_kinds_wide.hip).  Plain inlined functions: a kernel that uses one compiles to the
// instructions it had with the text written out (profiles/r19 holds the comparison, and the helpers that did not pass it).
#pragma once
#include "lo_internal.h"

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

// ---- what the kernels of the rational-quadratic / periodic kind share (lo_kernel_param.hip, lo_kernel_kinds_wide.hip) -----
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

// ---- what the kernels of the spectral mixture kind share (lo_kernel_sm.hip, lo_kernel_kinds_wide.hip) --------------------
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
