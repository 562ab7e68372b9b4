// lo_kernel_fn.h -- the covariance families of LO_OP_KERNEL_DIAG as functions of r^2 (lo_amd.h LO_KERNEL_*), shared by
// the on-the-fly product (lo_kernel_op.hip) and the row source of the pivoted Cholesky (lo_pivchol.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lo_amd.h"

namespace lo {

constexpr float kKfLog2e = 1.44269504088896340736f;
constexpr float kKfSqrt3 = 1.73205080756887729353f;
constexpr float kKfSqrt5 = 2.23606797749978969641f;
// beyond this r^2 every family is 0 in fp32 (exp(-sqrt(1e30)) underflows); the clamp keeps polynomial x exp finite
constexpr float kKfMaxR2 = 1e30f;

// exp(x) for x <= 0 as one v_exp_f32 on the argument multiplied by log2(e) beforehand: `xl` = x log2(e)
__device__ __forceinline__ float kf_exp2(float xl) { return __builtin_amdgcn_exp2f(xl); }

// g(r) from r^2 (FAMILY a compile-time constant in the hot loops): sqrt only for the Matern families
template <int FAMILY>
__device__ __forceinline__ float kf_g(float r2) {
  if constexpr (FAMILY == LO_KERNEL_RBF) {
    return kf_exp2(r2 * (-0.5f * kKfLog2e));
  } else {
    const float r = __builtin_amdgcn_sqrtf(fminf(r2, kKfMaxR2));
    if constexpr (FAMILY == LO_KERNEL_MATERN12) {
      return kf_exp2(r * -kKfLog2e);
    } else if constexpr (FAMILY == LO_KERNEL_MATERN32) {
      return fmaf(kKfSqrt3, r, 1.0f) * kf_exp2(r * (-kKfSqrt3 * kKfLog2e));
    } else {
      const float poly = fmaf(5.0f / 3.0f, fminf(r2, kKfMaxR2), fmaf(kKfSqrt5, r, 1.0f));
      return poly * kf_exp2(r * (-kKfSqrt5 * kKfLog2e));
    }
  }
}

// g(r) and h(r) = g'(r) / r, the factor of d r^2 / 2 in the derivative of g: dg = h (d r^2) / 2.  Finite at r = 0 for
// every family but Matern-1/2, whose h = -g / r is taken as 0 there (the pair adds nothing; no division by r).
template <int FAMILY>
__device__ __forceinline__ void kf_gh(float r2, float* g, float* h) {
  if constexpr (FAMILY == LO_KERNEL_RBF) {
    const float e = kf_exp2(r2 * (-0.5f * kKfLog2e));
    *g = e;
    *h = -e;
  } else {
    const float r2c = fminf(r2, kKfMaxR2);
    const float r = __builtin_amdgcn_sqrtf(r2c);
    if constexpr (FAMILY == LO_KERNEL_MATERN12) {
      const float e = kf_exp2(r * -kKfLog2e);
      *g = e;
      *h = r2c > 1e-30f ? -e * __builtin_amdgcn_rsqf(r2c) : 0.0f;  // (below: h r^2 < 1e-15, and rsq of a denormal is inf)
    } else if constexpr (FAMILY == LO_KERNEL_MATERN32) {
      const float e = kf_exp2(r * (-kKfSqrt3 * kKfLog2e));
      *g = fmaf(kKfSqrt3, r, 1.0f) * e;
      *h = -3.0f * e;
    } else {
      const float e = kf_exp2(r * (-kKfSqrt5 * kKfLog2e));
      *g = fmaf(5.0f / 3.0f, r2c, fmaf(kKfSqrt5, r, 1.0f)) * e;
      *h = (-5.0f / 3.0f) * fmaf(kKfSqrt5, r, 1.0f) * e;
    }
  }
}

// The float64 pair functions (lo_kernel_op_f64.hip).  There is no hardware double-precision exponential: exp and sqrt are
// the device math library's.  The Matern families clamp r^2 at kKfMaxR2D, so that polynomial x exp stays finite (and is
// 0) when r^2 overflows; RBF needs no clamp, exp(-inf) is 0.
constexpr double kKfSqrt3D = 1.7320508075688772935274463415058723669428;
constexpr double kKfSqrt5D = 2.2360679774997896964091736687312762354406;
constexpr double kKfMaxR2D = 1e300;
constexpr double kKfR2FloorD = 1e-30;  // covariance._R2_FLOOR: a closer pair adds nothing to the Matern-1/2 derivatives

template <int FAMILY>
__device__ __forceinline__ double kf_g64(double r2) {
  if constexpr (FAMILY == LO_KERNEL_RBF) {
    return exp(-0.5 * r2);
  } else {
    const double r2c = fmin(r2, kKfMaxR2D);
    const double r = sqrt(r2c);
    if constexpr (FAMILY == LO_KERNEL_MATERN12) {
      return exp(-r);
    } else if constexpr (FAMILY == LO_KERNEL_MATERN32) {
      return fma(kKfSqrt3D, r, 1.0) * exp(-kKfSqrt3D * r);
    } else {
      return fma(5.0 / 3.0, r2c, fma(kKfSqrt5D, r, 1.0)) * exp(-kKfSqrt5D * r);
    }
  }
}

// g(r) and h(r) = g'(r) / r in float64, as kf_gh: h of Matern-1/2 is taken as 0 for r^2 <= kKfR2FloorD
template <int FAMILY>
__device__ __forceinline__ void kf_gh64(double r2, double* g, double* h) {
  if constexpr (FAMILY == LO_KERNEL_RBF) {
    const double e = exp(-0.5 * r2);
    *g = e;
    *h = -e;
  } else {
    const double r2c = fmin(r2, kKfMaxR2D);
    const double r = sqrt(r2c);
    if constexpr (FAMILY == LO_KERNEL_MATERN12) {
      const double e = exp(-r);
      *g = e;
      *h = r2c > kKfR2FloorD ? -e / r : 0.0;
    } else if constexpr (FAMILY == LO_KERNEL_MATERN32) {
      const double e = exp(-kKfSqrt3D * r);
      *g = fma(kKfSqrt3D, r, 1.0) * e;
      *h = -3.0 * e;
    } else {
      const double e = exp(-kKfSqrt5D * r);
      *g = fma(5.0 / 3.0, r2c, fma(kKfSqrt5D, r, 1.0)) * e;
      *h = (-5.0 / 3.0) * fma(kKfSqrt5D, r, 1.0) * e;
    }
  }
}

// The pair function of the gradient kernel (LO_OP_KERNEL_GRAD_DIAG): for k = os2 g with g a function of r^2 and u the
// scaled difference, the block of a pair is g0, t_b u_b g1, -t_a u_a g1, t_a t_b (delta_ab g1 - u_a u_b g2) with
// g0 = g, g1 = -2 dg / d(r^2), g2 = 4 d^2 g / d(r^2)^2.  RBF: g0 = g1 = g2 = exp(-r^2 / 2), ONE factor, which is all
// the callers use today; a twice differentiable family (Matern-5/2) adds its case here and the callers take three.
template <int FAMILY>
__device__ __forceinline__ float kf_grad_pair(float r2) {
  static_assert(FAMILY == LO_KERNEL_RBF, "the gradient kernel is built for RBF only");
  return kf_g<LO_KERNEL_RBF>(r2);
}

// ---- the families with a shape parameter (LO_OP_KERNEL_PARAM_DIAG: lo_kernel_param.hip, lo_pivchol.hip) -----------------
// Rational quadratic, g = (1 + q)^(-alpha) with q = r^2 / (2 alpha): one v_log_f32 and one v_exp_f32, alpha and
// inv2a = 1 / (2 alpha) uniform over the workgroup.  The clamp keeps q / (1 + q) finite when r^2 overflows.
constexpr float kKpLn2 = 0.69314718055994530942f;
// d g / d alpha = g (q / (1 + q) - ln(1 + q)) cancels to -q^2 / 2 for small q.  Below this q the series -q^2 / 2 + 2 q^3 / 3 -
// 3 q^4 / 4 is used: its truncation error 4 q^5 / 5 relative to q^2 / 2 is 1.6 q^3 = 4.9e-5 at the threshold, where the
// direct form has 2^-23 / q^2 = 1.2e-4 (1 + q rounds by 2^-24, against q^2 / 2); the two errors cross at q = 0.038.
constexpr float kKpSeriesQ = 0.03125f;

__device__ __forceinline__ float kp_rq_g(float r2, float alpha, float inv2a) {
  const float q = fminf(r2, kKfMaxR2) * inv2a;
  return kf_exp2(-alpha * __builtin_amdgcn_logf(1.0f + q));
}

// g, h = g'(r) / r = -g / (1 + q) (the factor kf_gh gives) and ga = d g / d alpha
__device__ __forceinline__ void kp_rq_gha(float r2, float alpha, float inv2a, float* g, float* h, float* ga) {
  const float q = fminf(r2, kKfMaxR2) * inv2a;
  const float l2 = __builtin_amdgcn_logf(1.0f + q);
  const float rc = __builtin_amdgcn_rcpf(1.0f + q);
  const float e = kf_exp2(-alpha * l2);
  *g = e;
  *h = -e * rc;
  const float series = q * q * fmaf(q, fmaf(q, -0.75f, 2.0f / 3.0f), -0.5f);
  *ga = e * (q < kKpSeriesQ ? series : fmaf(q, rc, -l2 * kKpLn2));
}

// Periodic: sin(pi p) and sin(2 pi p) for p = |phi| >= 0 (the callers take |phi|, so that K(x, y) and K(y, x) have equal
// bits, and put the sign back where the function is odd).  v_sin_f32 takes revolutions and a bounded domain: fract first,
// which is exact at any magnitude.
#ifndef LO_KP_HW_SINE
#define LO_KP_HW_SINE 1
#endif
__device__ __forceinline__ float kp_sinpi(float p) {
#if LO_KP_HW_SINE
  return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(0.5f * p));
#else
  return sinpif(p);
#endif
}
__device__ __forceinline__ float kp_sin2pi(float p) {
#if LO_KP_HW_SINE
  return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(p));
#else
  return sinpif(2.0f * p);
#endif
}
// g = exp(-2 rho), rho = sum_k (theta_k sin(pi phi_k))^2
__device__ __forceinline__ float kp_per_g(float rho) { return kf_exp2(rho * (-2.0f * kKfLog2e)); }

// one entry with everything a run-time value (row source of the pivoted Cholesky): theta [2 D + 2] as lo_amd.h lays it
// out; the points scaled and rounded separately, then differenced, the sums in ascending k
__device__ __forceinline__ float kp_g_rt(int family, const float* xp, const float* xi, const float* th, int D) {
  float acc = 0.0f;
  if (family == LO_KERNEL_PERIODIC) {
    const float* nu = th + D + 2;
    for (int k = 0; k < D; ++k) {
      const float ts = th[k] * kp_sinpi(fabsf(xp[k] * nu[k] - xi[k] * nu[k]));
      acc = acc + ts * ts;
    }
    return kp_per_g(acc);
  }
  for (int k = 0; k < D; ++k) {
    const float df = xp[k] * th[k] - xi[k] * th[k];
    acc = acc + df * df;
  }
  return kp_rq_g(acc, th[D + 1], 0.5f / th[D + 1]);
}

// ---- the spectral mixture kernel (LO_OP_KERNEL_SM_DIAG: lo_kernel_sm.hip, lo_pivchol.hip) -------------------------------
// k = sum_q w_q exp(-2 pi^2 sum_k (sigma_qk tau_k)^2) prod_k cos(2 pi mu_qk tau_k), tau = x - x'.  cos(2 pi p) for
// p = |mu tau| >= 0 in revolutions: fract first (exact at any magnitude), then v_cos_f32, as kp_sin2pi; its sine partner in
// the derivatives is kp_sin2pi itself.
#ifndef LO_KSM_HW_COSINE
#define LO_KSM_HW_COSINE 1
#endif
__device__ __forceinline__ float ksm_cos2pi(float p) {
#if LO_KSM_HW_COSINE
  return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(p));
#else
  return cospif(2.0f * p);
#endif
}
constexpr float kKsmPi = 3.14159265358979323846f;
constexpr float kKsmExpScale = -2.0f * kKsmPi * kKsmPi * kKfLog2e;  // E = exp2(kKsmExpScale sum_k (sigma_k tau_k)^2)
__device__ __forceinline__ float ksm_env(float s2) { return kf_exp2(s2 * kKsmExpScale); }

// one entry with everything a run-time value (row source of the pivoted Cholesky): theta [Q, 2 D + 1] as lo_amd.h lays it
// out (w, mu_1 .. mu_D, sigma_1 .. sigma_D per mixture); the points differenced first, the sums in ascending k and q
__device__ __forceinline__ float ksm_g_rt(const float* xp, const float* xi, const float* th, int D, int Q) {
  float acc = 0.0f;
  for (int q = 0; q < Q; ++q) {
    const float* t = th + (size_t)q * (2 * D + 1);
    float s2 = 0.0f, pr = 1.0f;
    for (int k = 0; k < D; ++k) {
      const float tau = fabsf(xp[k] - xi[k]);
      const float st = t[1 + D + k] * tau;
      s2 = s2 + st * st;
      pr = pr * ksm_cos2pi(fabsf(t[1 + k]) * tau);
    }
    const float term = t[0] * (ksm_env(s2) * pr);
    acc = q == 0 ? term : acc + term;
  }
  return acc;
}

// the same with the family as a run-time value (row source of the pivoted Cholesky: one entry per thread)
__device__ __forceinline__ float kf_g_rt(int family, float r2) {
  switch (family) {
    case LO_KERNEL_RBF: return kf_g<LO_KERNEL_RBF>(r2);
    case LO_KERNEL_MATERN12: return kf_g<LO_KERNEL_MATERN12>(r2);
    case LO_KERNEL_MATERN32: return kf_g<LO_KERNEL_MATERN32>(r2);
    default: return kf_g<LO_KERNEL_MATERN52>(r2);
  }
}

}  // namespace lo
