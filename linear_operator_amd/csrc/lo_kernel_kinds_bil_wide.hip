// lo_kernel_kinds_bil_wide.hip -- the derivatives of sum_s u_s^T K(x1, x2) v_s for MANY columns s of the matrix-free kinds
// with a pair value of their own (ABI 47): rational quadratic and periodic (lo_kernel_param.hip) and spectral mixture
// (lo_kernel_sm.hip).  lo_kernel_param_bilinear_wide_f32, lo_kernel_param_points_grad_wide_f32,
// lo_kernel_sm_bilinear_wide_f32, lo_kernel_sm_points_grad_wide_f32 and the branches of kernel_param_bil_run /
// kernel_param_pgrad_run / kernel_sm_bil_run / kernel_sm_pgrad_run that kp_bil_wide / ksm_bil_wide select
// (lo_kernel_shape.h).  K is never in memory.
//
// k_kparam_bil / k_kparam_pgrad and k_ksm_bil / k_ksm_pgrad form W_ij = sum_s U_is V_js with kKoTS = 8 vector FMAs per pair
// and form every value and derivative factor -- a logarithm and an exponential, D sines, or Q D sines and cosines and Q
// exponentials -- again in the next sweep of 8 columns.  Here W = U V^T runs on v_mfma_f32_32x32x2_f32 (exact fp32
// products, fp32 accumulation), up to 32 columns per sweep, and the pair work happens once per pair and sweep, by the
// device functions and in the operation order of those kernels.
//
// The frame is k_kernel_bil_wide's (lo_kernel_bil_wide.hip), one body for the three families:
//   split      256 threads own 256 rows of one member (KoSweep, ko_shape, split-j over gridDim.z; kp_bil_layout /
//              ksm_bil_layout with k_kparam_bil_reduce / k_ksm_bil_reduce for the hyperparameters, ko_split_layout /
//              ko_reduce_splits for the points, all unchanged); a wave owns 64 rows as two 32-row tiles tau = 0, 1
//   W          per block of 32 points j of the LDS tile and per row tile W^T[32 j x 32 i] += V^T[32 j x 2 s] U^T[2 s x 32 i].
//              In lane l (li = l % 32, h = l / 32) the A operand is V[jb + li][s + h] from LDS (s-major, row stride 160
//              words: the two halves of a wave fall into disjoint halves of the 64 banks), the B operand is
//              U[i0 + 32 tau + li][s + h], kept in registers for the sweep; ceil(cols / 2) steps, a wave-uniform bound
//   rows       v_permlane32_swap_b32 of acc0[r] and acc1[r] gives lane l row i0 + l: acc0[r] is then point
//              jb + 8 (r / 4) + r % 4 and acc1[r] point jb + 8 (r / 4) + 4 + r % 4.  The lane keeps ONE staged point a[DP]
//              and every read of the point tile is one wave-uniform address
//   pairs      in ascending j, w from an accumulator register.  For j >= nj of a ragged block the point read is clamped to
//              the tile's last valid one and w is SELECTED to 0; rows beyond M carry zero U and store nothing; a wave whose
//              64 rows lie beyond M stages, waits at the barriers and computes nothing
//   summation  tile sums added to running sums, block_sum256 and one partial per workgroup; a per-row store for the
//              points.  The one-number-per-member entries (os2, alpha, the mixture weight) are sums of N M terms of both
//              signs whose lane and wave sums are 10 - 1000 times the result: a lane adds their exact products in float64
//              and the workgroup adds the lanes in float64 (block_sum256_d), so the partial is rounded to float32 ONCE
//              (the one-lane kernels: a compensated float32 sum per lane, then float32 block sums whose roundings, each
//              half an ulp of a sum far larger than the result, were most of the slot's error where DESIGN.md section 6zc
//              took it apart).  No atomics, no workgroup waits for another: two calls give equal bits
// What differs per family is a policy (below): what of theta sits in LDS, how a point is staged, which row block and which
// partial a workgroup owns, the sums a lane keeps and what one pair adds to them.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using kbw_f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kKbwStride = kKoTJ + 32;  // words between two columns s of the V tile (see above)

// Rational quadratic and periodic.  LDS: th[DP] = t_k, sc[DP] = what the points are scaled by (RQ: t_k, PERIODIC: nu_k).
// The pair is kp_pair; the sums, their order and the partial's slots are those of k_kparam_bil / k_kparam_pgrad.
template <int FAMILY, int DP_>
struct KbwParam {
  static constexpr int DP = DP_;
  static constexpr bool PER = FAMILY == LO_KERNEL_PERIODIC;
  static constexpr int DQ = PER ? DP : 1;  // the period sums exist for PERIODIC only
  static constexpr int kCols = kp_bil_wide_cols(FAMILY, DP);
  static constexpr bool kRolled = false;  // the 32 pairs of a block unrolled, as in k_kernel_bil_wide
  static constexpr int words(bool) { return 2 * DP; }
  float *th, *sc;
  float os2, alpha, inv2a;

  template <bool POINTS>
  struct Sums {
    float run[DP], tile[DP];                                // lengthscales (POINTS: the coordinates of the gradient)
    float prun[POINTS ? 1 : DQ], ptile[POINTS ? 1 : DQ];    // periods
    double gos = 0.0, gal = 0.0;                            // os2 and alpha: one number per member each
  };

  // the member's theta into `tl` (ends with a barrier); returns the workgroup's row block
  template <bool POINTS>
  __device__ __forceinline__ int load(const float* __restrict__ theta, int64_t b, int D, int, float* tl) {
    const float* tb = theta + b * (2 * D + 2);
    th = tl;
    sc = tl + DP;
    kp_load_theta<FAMILY, DP>(tb, D, th, sc);
    os2 = tb[D];
    alpha = tb[D + 1];
    inv2a = 0.5f / alpha;
    return blockIdx.x;
  }
  __device__ __forceinline__ float point(float x, int k) const { return x * sc[k]; }
  __device__ __forceinline__ void stage(const float* __restrict__ x2b, int D, int jt, int nj, float* xs) const {
    ko_stage_points<DP>(x2b, sc, D, jt, nj, xs);
  }
  template <bool POINTS>
  __device__ __forceinline__ void begin(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.run[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < (POINTS ? 1 : DQ); ++k) s.prun[k] = 0.0f;
  }
  template <bool POINTS>
  __device__ __forceinline__ void tile_begin(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.tile[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < (POINTS ? 1 : DQ); ++k) s.ptile[k] = 0.0f;
  }
  template <bool POINTS>
  __device__ __forceinline__ void pair(Sums<POINTS>& s, const float (&a)[DP], const float* __restrict__ bp, float w) const {
    float e1[DP], e2[DP];
    float g, h, ga;
    kp_pair<FAMILY, DP, POINTS>(a, bp, th, alpha, inv2a, &g, &h, &ga, e1, e2);
    if constexpr (POINTS) {
      const float wf = w * (PER ? g : h);
#pragma unroll
      for (int k = 0; k < DP; ++k) s.tile[k] = fmaf(wf, PER ? e2[k] : e1[k], s.tile[k]);
    } else {
      s.gos = fma((double)w, (double)g, s.gos);
      if constexpr (PER) {
        const float wg = w * g;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          s.tile[k] = fmaf(wg, e1[k], s.tile[k]);
          s.ptile[k] = fmaf(wg, e2[k], s.ptile[k]);
        }
      } else {
        s.gal = fma((double)w, (double)ga, s.gal);
        const float wh = w * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) s.tile[k] = fmaf(wh * e1[k], e1[k], s.tile[k]);
      }
    }
  }
  template <bool POINTS>
  __device__ __forceinline__ void tile_end(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.run[k] += s.tile[k];
    if constexpr (PER && !POINTS) {
#pragma unroll
      for (int k = 0; k < DP; ++k) s.prun[k] += s.ptile[k];
    }
  }
  // the gradient of row i, coordinate k, with today's factors
  __device__ __forceinline__ float point_grad(const Sums<true>& s, int k) const {
    return PER ? (-2.0f * kKpPi) * os2 * th[k] * th[k] * sc[k] * s.run[k] : os2 * th[k] * s.run[k];
  }
  // one partial [2 DP + 2] per workgroup, part [B, nblk = gridDim.x * gridDim.z, 2 DP + 2], in today's slot order
  __device__ __forceinline__ void partial(const Sums<false>& s, int64_t b, int, float* __restrict__ part,
                                          float* red, double* redd) const {
    const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
    float* out = part + ((size_t)b * nblk + blk) * (2 * DP + 2);
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float sum = block_sum256(s.run[k], red);
      if (threadIdx.x == 0) out[k] = sum;
    }
    {
      const float sum = (float)block_sum256_d(s.gos, redd);
      if (threadIdx.x == 0) out[DP] = sum;
    }
    {
      const float sum = (float)block_sum256_d(s.gal, redd);
      if (threadIdx.x == 0) out[DP + 1] = sum;
    }
    if constexpr (PER) {  // (RQ: the period slots are never read)
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const float sum = block_sum256(s.prun[k], red);
        if (threadIdx.x == 0) out[DP + 2 + k] = sum;
      }
    }
  }
};

// Spectral mixture; the points stay raw.
//   hyperparameters  the grid of k_ksm_bil, blockIdx.x = row block * Q + q: one mixture per workgroup, |mu_q| and sigma_q in
//                    LDS, ksm_mixture with sines, ksm_leave_one_out, the sum for w compensated, 2 DP + 1 sums.  W is
//                    formed again by every mixture's workgroup: ceil(t / 2) matrix instructions per 32 x 32 pairs
//                    against DP sines and cosines per pair
//   points           the member's whole theta in LDS (ksm_load_theta) and the q loop inside the pair, as in k_ksm_pgrad
template <int DP_>
struct KbwSm {
  static constexpr int DP = DP_;
  static constexpr int kCols = ksm_bil_wide_cols(DP);
  static constexpr bool kRolled = true;  // one pair per trip (see the kernel): unrolled, the points' kernel spills
  static constexpr int words(bool points) { return points ? 2 * kKsmQ * DP + kKsmQ : 2 * DP; }
  float *mu, *sg, *tw;  // hyperparameters: [DP] of mixture q; points: [Q][DP] and tw[Q]
  int Q, q;

  template <bool POINTS>
  struct Sums {
    float run[DP], tile[DP];                                // mu (POINTS: the coordinates of the gradient)
    float prun[POINTS ? 1 : DP], ptile[POINTS ? 1 : DP];    // sigma
    double gw = 0.0;  // the weight: one number per member and mixture (see KbwParam)
  };

  template <bool POINTS>
  __device__ __forceinline__ int load(const float* __restrict__ theta, int64_t b, int D, int Q_, float* tl) {
    Q = Q_;
    if constexpr (POINTS) {
      q = 0;
      mu = tl;
      sg = tl + kKsmQ * DP;
      tw = tl + 2 * kKsmQ * DP;
      ksm_load_theta<DP>(theta + b * Q * (2 * D + 1), D, Q, tw, mu, sg);
      return blockIdx.x;
    } else {
      const int rblk = blockIdx.x / Q;
      q = blockIdx.x - rblk * Q;
      mu = tl;
      sg = tl + DP;
      tw = nullptr;
      if (threadIdx.x < DP) {
        const int k = threadIdx.x;
        const float* tq = theta + ((size_t)b * Q + q) * (2 * D + 1);
        mu[k] = k < D ? fabsf(tq[1 + k]) : 0.0f;
        sg[k] = k < D ? tq[1 + D + k] : 0.0f;
      }
      __syncthreads();
      return rblk;
    }
  }
  __device__ __forceinline__ float point(float x, int) const { return x; }
  __device__ __forceinline__ void stage(const float* __restrict__ x2b, int D, int jt, int nj, float* xs) const {
    ksm_stage_points<DP>(x2b, D, jt, nj, xs);
  }
  template <bool POINTS>
  __device__ __forceinline__ void begin(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.run[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < (POINTS ? 1 : DP); ++k) s.prun[k] = 0.0f;
  }
  template <bool POINTS>
  __device__ __forceinline__ void tile_begin(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.tile[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < (POINTS ? 1 : DP); ++k) s.ptile[k] = 0.0f;
  }
  template <bool POINTS>
  __device__ __forceinline__ void pair(Sums<POINTS>& s, const float (&a)[DP], const float* __restrict__ bp, float w) const {
    if constexpr (POINTS) {
      float df[DP], tau[DP], pq[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        df[k] = a[k] - bp[k];
        tau[k] = fabsf(df[k]);
        pq[k] = 0.0f;
      }
      // pq[k] = sum_q w_q E_q (2 pi sigma_qk^2 tau_k prod c + |mu_qk| s_k prod_{l != k} c_l); the factor -2 pi at the store
      for (int qq = 0; qq < Q; ++qq) {
        float c[DP], sn[DP], ex[DP];
        const float* m = mu + qq * DP;
        const float* g = sg + qq * DP;
        const float E = ksm_mixture<DP, true>(tau, m, g, c, sn);
        const float pr = ksm_leave_one_out<DP>(c, ex);
        const float wE = tw[qq] * E;
        const float wEp = (2.0f * kKsmPi) * wE * pr;
#pragma unroll
        for (int k = 0; k < DP; ++k) pq[k] = fmaf(wEp * (g[k] * g[k]), tau[k], fmaf(wE * (m[k] * sn[k]), ex[k], pq[k]));
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) s.tile[k] = fmaf(df[k] < 0.0f ? -w : w, pq[k], s.tile[k]);
    } else {
      float tau[DP], c[DP], sn[DP], ex[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) tau[k] = fabsf(a[k] - bp[k]);
      const float E = ksm_mixture<DP, true>(tau, mu, sg, c, sn);
      const float pr = ksm_leave_one_out<DP>(c, ex);
      const float wE = w * E;
      s.gw = fma((double)wE, (double)pr, s.gw);
      const float wEp = wE * pr;
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        s.ptile[k] = fmaf(wEp, tau[k] * tau[k], s.ptile[k]);
        s.tile[k] = fmaf(wE * (tau[k] * sn[k]), ex[k], s.tile[k]);
      }
    }
  }
  template <bool POINTS>
  __device__ __forceinline__ void tile_end(Sums<POINTS>& s) const {
#pragma unroll
    for (int k = 0; k < DP; ++k) s.run[k] += s.tile[k];
    if constexpr (!POINTS) {
#pragma unroll
      for (int k = 0; k < DP; ++k) s.prun[k] += s.ptile[k];
    }
  }
  __device__ __forceinline__ float point_grad(const Sums<true>& s, int k) const { return (-2.0f * kKsmPi) * s.run[k]; }
  // one partial [2 DP + 1] per workgroup, part [B, Q, nblk = row blocks * gridDim.z, 2 DP + 1]: slot 0 the sum for w,
  // 1 + k for mu_k, 1 + DP + k for sigma_k (all without their factors: k_ksm_bil_reduce)
  __device__ __forceinline__ void partial(const Sums<false>& s, int64_t b, int rblk, float* __restrict__ part,
                                          float* red, double* redd) const {
    const int nrb = gridDim.x / Q;
    const size_t blk = (size_t)blockIdx.z * nrb + rblk, nblk = (size_t)nrb * gridDim.z;
    float* out = part + (((size_t)b * Q + q) * nblk + blk) * (2 * DP + 1);
    {
      const float sum = (float)block_sum256_d(s.gw, redd);
      if (threadIdx.x == 0) out[0] = sum;
    }
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float sum = block_sum256(s.run[k], red);
      if (threadIdx.x == 0) out[1 + k] = sum;
    }
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float sum = block_sum256(s.prun[k], red);
      if (threadIdx.x == 0) out[1 + DP + k] = sum;
    }
  }
};

// grid (row blocks [* Q: spectral mixture, hyperparameters], B, js).  POINTS false: out is the policy's partials; POINTS
// true: out is g_x1 [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D] of the column splits.
// Q: the mixtures of the spectral mixture kind (the other policy ignores it).
template <class POL, bool POINTS>
__global__ __launch_bounds__(kThreads) void k_kinds_bil_wide(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             const float* __restrict__ theta, int Q, int M, int N, int D,
                                                             const float* __restrict__ U, const float* __restrict__ V,
                                                             int t, float* __restrict__ out, int jchunk) {
  constexpr int DP = POL::DP, CH = POL::kCols;  // CH: columns s per sweep (even)
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[CH * kKbwStride];
  __shared__ __align__(16) float tl[POL::words(POINTS)];
  __shared__ float red[4];
  __shared__ double redd[4];
  const int64_t b = blockIdx.y;
  POL pol;
  const int rblk = pol.template load<POINTS>(theta, b, D, Q, tl);
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const int i0 = rblk * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  const int i = i0 + lane;                                   // the row whose pairs this lane sums
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (i < M && k < D) ? pol.point(x1[((size_t)b * M + i) * D + k], k) : 0.0f;
  typename POL::template Sums<POINTS> sums;
  pol.template begin<POINTS>(sums);
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += CH) {
    const int steps = (min(CH, t - s0) + 1) / 2;  // contraction steps of this sweep: two columns each
    float ub[2][CH / 2];                          // the B operands: U[i0 + 32 tau + li][s0 + 2 step + h]
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
      const int iu = i0 + 32 * tau + li;
#pragma unroll
      for (int q = 0; q < CH / 2; ++q) {
        const int s = s0 + 2 * q + h;
        ub[tau][q] = (iu < M && s < t) ? U[((size_t)b * M + iu) * t + s] : 0.0f;
      }
    }
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      pol.stage(x2b, D, jt, nj, xs);
      for (int e = threadIdx.x; e < 2 * steps * kKoTJ; e += kThreads) {  // (the rows the MFMA steps read, all 128 j)
        const int ss = e / kKoTJ, j = e - ss * kKoTJ;
        vs[ss * kKbwStride + j] = (j < nj && s0 + ss < t) ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      if (i0 >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
      pol.template tile_begin<POINTS>(sums);  // (a tile's sums on their own, then added to the running ones, as in the product)
      for (int jb = 0; jb < nj; jb += 32) {
        kbw_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
        const float* ap = vs + h * kKbwStride + jb + li;
#pragma unroll
        for (int q = 0; q < CH / 2; ++q)
          if (q < steps) {
            const float av = ap[2 * q * kKbwStride];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ub[0][q], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ub[1][q], acc1, 0, 0, 0);
          }
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // rows i0 + 32 .. 63 of tile 1 to the upper half wave, its points 4 .. 7 to tile 1
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc0[r]), __float_as_uint(acc1[r]), false, false);
          acc0[r] = __uint_as_float(sw[0]);
          acc1[r] = __uint_as_float(sw[1]);
        }
        auto pair = [&](int j, float wr) {  // j: wave uniform
          pol.template pair<POINTS>(sums, a, xs + min(j, nj - 1) * DP, j < nj ? wr : 0.0f);
        };
        // ascending j: points 8 q .. 8 q + 3 in acc0, 8 q + 4 .. 8 q + 7 in acc1
        if constexpr (POL::kRolled) {
          // One pair per trip: 32 unrolled pairs let the sines and cosines of all of them overlap, which costs up to 2.9 KB
          // of scratch per lane.  A trip takes its w from register (0, 0); the eight of a q move down by one after every
          // pair, the q by one after every eight (as section 6za rolled its pairs).
          float wq[4][8];
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 0; m < 4; ++m) wq[q][m] = acc0[4 * q + m], wq[q][4 + m] = acc1[4 * q + m];
#pragma unroll 1
          for (int q = 0; q < 4; ++q) {
#pragma unroll 1
            for (int m = 0; m < 8; ++m) {
              pair(jb + 8 * q + m, wq[0][0]);
#pragma unroll
              for (int e = 0; e < 7; ++e) wq[0][e] = wq[0][e + 1];
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) wq[0][e] = wq[1][e], wq[1][e] = wq[2][e], wq[2][e] = wq[3][e];
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int m = 0; m < 4; ++m) pair(jb + 8 * q + m, acc0[4 * q + m]);
#pragma unroll
            for (int m = 0; m < 4; ++m) pair(jb + 8 * q + 4 + m, acc1[4 * q + m]);
          }
        }
      }
      pol.template tile_end<POINTS>(sums);
    }
  }
  if constexpr (POINTS) {
    if (i < M) {
      float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
      for (int k = 0; k < DP; ++k)
        if (k < D) o[k] = pol.point_grad(sums, k);
    }
  } else {
    pol.partial(sums, b, rblk, out, red, redd);
  }
}

// f(policy) for the family's instantiation, as an empty tag value
template <class POL>
struct KbwTag {
  using type = POL;
};
template <class F>
static void kbw_param_pick(int family, int DP, F&& f) {
  kp_dispatch(family, DP, [&](auto fam, auto dp) { f(KbwTag<KbwParam<fam(), dp()>>{}); });
}
template <class F>
static void kbw_sm_pick(int DP, F&& f) {
  ko_pick(ksm_dims{}, DP, [&](auto dp) { f(KbwTag<KbwSm<dp()>>{}); });
}

template <bool POINTS, class TAG>
static void kbw_launch(TAG, dim3 grid, const float* x1, const float* x2, const float* theta, int64_t Q, int64_t M,
                       int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* out, int jchunk,
                       hipStream_t st) {
  hipLaunchKernelGGL((k_kinds_bil_wide<typename TAG::type, POINTS>), grid, dim3(kThreads), 0, st, x1, x2, theta, (int)Q,
                     (int)M, (int)N, (int)D, U, V, (int)t, out, jchunk);
}

// the points' gradient of either kind: `pick(f)` calls f with the family's tag
template <class PICK>
static int kbw_pgrad_run(const char* reduce_name, PICK&& pick, const float* x1, const float* x2, const float* theta,
                         int64_t Q, int64_t B, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                         float* g_x1, float* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_kinds_pgrad_wide", st);
  pick(w.DP, [&](auto tag) { kbw_launch<true>(tag, w.grid, x1, x2, theta, Q, M, N, D, U, V, t, out, w.s.jchunk, st); });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko_reduce_splits(reduce_name, part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr, LO_DIAG_NONE,
                            nullptr, g_x1, nullptr, st);
  return LO_OK;
}

int kernel_param_bil_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta,
                              float* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kinds_bil_wide", st);
  kbw_param_pick(family, w.DP, [&](auto tag) {
    kbw_launch<false>(tag, w.grid, x1, x2, theta, 0, M, N, D, U, V, t, part, w.s.jchunk, st);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return kp_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, family, theta, g_theta, st);
}

int kernel_param_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                                int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                                hipStream_t st) {
  return kbw_pgrad_run("k_kparam_pgrad_wide_reduce", [&](int DP, auto&& f) { kbw_param_pick(family, DP, f); }, x1, x2,
                       theta, 0, B, M, N, D, U, V, t, g_x1, part, st);
}

int kernel_sm_bil_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                           int64_t D, const float* U, const float* V, int64_t t, float* g_theta, float* part,
                           hipStream_t st) {
  const KoSweep w(B, M, N, D);
  const dim3 grid((unsigned)(w.s.rb * Q), (unsigned)B, (unsigned)w.s.js);  // (rb <= 2^23, Q <= 16)
  LO_PROF_BEGIN("k_kinds_bil_wide", st);
  kbw_sm_pick(w.DP, [&](auto tag) {
    kbw_launch<false>(tag, grid, x1, x2, theta, Q, M, N, D, U, V, t, part, w.s.jchunk, st);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return ksm_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, Q, theta, g_theta, st);
}

int kernel_sm_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                             int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                             hipStream_t st) {
  return kbw_pgrad_run("k_ksm_pgrad_wide_reduce", [&](int DP, auto&& f) { kbw_sm_pick(DP, f); }, x1, x2, theta, Q, B, M, N,
                       D, U, V, t, g_x1, part, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_param_bilinear_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { kp_bil_layout(ar, B, M, N, D); });
}

int lo_kernel_param_bilinear_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                      int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                      float* g_theta, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !kp_family_ok(family))
    return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = kp_bil_layout(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_param_bil_wide_run(x1, x2, theta, family, B, M, N, D, U, V, t, g_theta, part, (hipStream_t)stream);
}

size_t lo_kernel_param_points_grad_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_param_points_grad_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                         int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                         float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !kp_family_ok(family))
    return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_param_pgrad_wide_run(x1, x2, theta, family, B, M, N, D, U, V, t, g_x1, part, (hipStream_t)stream);
}

size_t lo_kernel_sm_bilinear_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t) {
  if (!ksm_args_ok(B, M, N, D, Q, t) || !ksm_shape_ok(B, M, N, D, Q, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ksm_bil_layout(ar, B, M, N, D, Q); });
}

int lo_kernel_sm_bilinear_wide_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                                   int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ksm_args_ok(B, M, N, D, Q, t)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, t)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ksm_bil_layout(ar, B, M, N, D, Q);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_sm_bil_wide_run(x1, x2, theta, Q, B, M, N, D, U, V, t, g_theta, part, (hipStream_t)stream);
}

size_t lo_kernel_sm_points_grad_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t t) {
  if (!ksm_args_ok(B, M, N, D, Q, t) || !ksm_shape_ok(B, M, N, D, Q, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_sm_points_grad_wide_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B,
                                      int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                      float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ksm_args_ok(B, M, N, D, Q, t)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, t)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_sm_pgrad_wide_run(x1, x2, theta, Q, B, M, N, D, U, V, t, g_x1, part, (hipStream_t)stream);
}

}  // extern "C"
