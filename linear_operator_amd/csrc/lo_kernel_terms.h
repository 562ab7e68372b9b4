// lo_kernel_terms.h -- the device pieces that the kinds with SEVERAL kernel terms over one point tensor share
// (lo_kernel_sum.hip: sum_t K_t; lo_kernel_lmc.hip: sum_q K_q (x) B_q): the tile of x2 staged once per term and scaled by
// that term's inverse lengthscales, the rounding of a scaled coordinate, the loop over the 8 pairs of a sub-tile as a
// template of the family, the switch on a term's family outside that loop, and the packed family codes.
#pragma once
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"

namespace lo {

constexpr int kKsJS = 8;   // pairs per sub-tile

// points of x2 per LDS tile: T copies of the tile are staged, so the widest points take half a tile of lo_kernel_op.hip
template <int DP>
constexpr int ks_tile() { return DP == 32 ? kKoTJ / 2 : kKoTJ; }

// A coordinate times the term's inverse lengthscale, rounded on its own.  The thread scales its point in registers and
// the staging loop scales the tile in LDS: both products must round alike, or coincident points would not give r = 0 -- a
// product contracted into the subtraction that follows it (one fused multiply-add) would leave the rounding residue.
__device__ __forceinline__ float ks_scale(float x, float th) {
  float p = x * th;
  asm volatile("" : "+v"(p));  // (no instruction: the product is opaque to the contraction of a * b - c)
  return p;
}

// th[tt][DP + 1] of the terms [t0, t0 + nt): the D inverse lengthscales (0 beyond D), os2 in slot DP
template <int DP>
__device__ __forceinline__ void ks_stage_theta(const float* __restrict__ theta_b, int D, int t0, int nt,
                                               float* __restrict__ th) {
  for (int e = threadIdx.x; e < nt * (DP + 1); e += kThreads) {
    const int tt = e / (DP + 1), k = e - tt * (DP + 1);
    const float* src = theta_b + (size_t)(t0 + tt) * (D + 1);
    th[e] = k < D ? src[k] : (k == DP ? src[D] : 0.0f);
  }
}

// the tile [jt, jt + nj) of x2 once per term, scaled by the term's inverse lengthscales: xs[tt][TJ][DP]; the rows
// [nj, njp) of a ragged sub-tile and the coordinates >= D are 0
template <int DP>
__device__ __forceinline__ void ks_stage_points(const float* __restrict__ x2b, const float* __restrict__ th, int D, int nt,
                                                int jt, int nj, int njp, float* __restrict__ xs) {
  constexpr int TJ = ks_tile<DP>();
  const int per = njp * DP;
  for (int e = threadIdx.x; e < nt * per; e += kThreads) {
    const int tt = e / per, r = e - tt * per;
    const int j = r / DP, k = r - j * DP;
    float s = 0.0f;
    if (j < nj && k < D) s = ks_scale(x2b[(size_t)(jt + j) * D + k], th[tt * (DP + 1) + k]);
    xs[((size_t)tt * TJ + j) * DP + k] = s;
  }
}

// kv[jj] += os2 g(r_jj) over the 8 pairs of a sub-tile, one instantiation per family
template <int FAMILY, int DP>
__device__ __forceinline__ void ks_sub_g(const float (&at)[DP], const float* __restrict__ xt, float os2,
                                         float (&kv)[kKsJS]) {
#pragma unroll
  for (int jj = 0; jj < kKsJS; ++jj) {
    float r2 = 0.0f;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float df = at[k] - xt[jj * DP + k];
      r2 = fmaf(df, df, r2);
    }
    kv[jj] = fmaf(os2, kf_g<FAMILY>(r2), kv[jj]);
  }
}

// the family of a term, uniform over the workgroup: switched on once per sub-tile
#define KS_FAMILY_SWITCH(fam_, CALL_)                            \
  switch (fam_) {                                                \
    case LO_KERNEL_RBF: CALL_(LO_KERNEL_RBF); break;             \
    case LO_KERNEL_MATERN12: CALL_(LO_KERNEL_MATERN12); break;   \
    case LO_KERNEL_MATERN32: CALL_(LO_KERNEL_MATERN32); break;   \
    default: CALL_(LO_KERNEL_MATERN52); break;                   \
  }

// a packed word (four bits per term, term 0 lowest) holds T known codes and nothing else
inline bool ks_packed_ok(int64_t packed, int64_t T) {
  if (packed < 0 || (packed >> (4 * T)) != 0) return false;
  for (int64_t t = 0; t < T; ++t)
    if (!ko_family_ok((packed >> (4 * t)) & 15)) return false;
  return true;
}

}  // namespace lo
