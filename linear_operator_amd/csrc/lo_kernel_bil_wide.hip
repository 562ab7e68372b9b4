// lo_kernel_bil_wide.hip -- the derivatives of sum_s u_s^T K(x1, x2) v_s for MANY columns s (ABI 43):
// lo_kernel_bilinear_wide_f32, lo_kernel_points_grad_wide_f32 and the branch of kernel_bil_run / kernel_pgrad_run that
// ko_bil_wide selects (lo_kernel_shape.h).  K is never in memory.
//
// k_kernel_bil and k_kernel_pgrad (lo_kernel_op.hip) form W_ij = sum_s U_is V_js with kKoTS = 8 vector FMAs per pair and
// form every r^2, g, h and s_d again in the next sweep of 8 columns.  Here W = U V^T, a GEMM with contraction length t, runs
// on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation), up to ko_bil_wide_cols(DP) columns per sweep, and the
// pair work -- direct differences, one exp, one sqrt -- happens once per pair and sweep.
//
// Split of work: that of k_kernel_bil / k_kernel_pgrad.  A workgroup is 256 threads and owns 256 rows of one member
//   (KoSweep, ko_shape, split-j over gridDim.z; ko_bil_layout / ko_bil_reduce for the hyperparameters, ko_split_layout /
//   ko_reduce_splits for the points).  A wave owns 64 rows as two 32-row tiles tau = 0, 1.
// W on the matrix cores, transposed: per block of 32 points j of the LDS tile and per row tile,
//   W^T[32 j x 32 i] += V^T[32 j x 2 s] U^T[2 s x 32 i].  In lane l (li = l % 32, h = l / 32) the A operand is
//   V[jb + li][s + h], read from LDS, the B operand is U[i0 + 32 tau + li][s + h], kept in registers for the whole sweep
//   (half the columns of the chunk for each of two rows); ceil(cols / 2) steps for the chunk's actual column count, a
//   wave-uniform bound.  Accumulator register r of tile tau is then W[i0 + 32 tau + li][jb + 8 (r / 4) + 4 h + r % 4] (the
//   layout of lo_kernel_mv_wide.hip and lo_chol.hip).
// One row per lane again: v_permlane32_swap_b32 exchanges lanes 32 - 63 of its first operand with lanes 0 - 31 of its
//   second.  With acc0[r] first and acc1[r] second, lane l owns row i0 + l -- the row mapping of the old kernels -- and in
//   every lane acc0[r] is point jb + 8 (r / 4) + r % 4, acc1[r] is point jb + 8 (r / 4) + 4 + r % 4: 16 swaps per 2048
//   pairs.  So the lane keeps ONE scaled point a[DP], and every read of the point tile xs is one wave-uniform address.
// Pair loop: the inner loop of the old kernels with w taken from an accumulator register, the points in ascending j.  For
//   j >= nj of a ragged block of 32 the point read is the tile's last valid one (a wave-uniform clamp of the index, so
//   nothing that xs holds behind the end is ever read) and w is SELECTED to 0, not multiplied.  Rows beyond M carry zero
//   U, so they add nothing and store nothing; a wave whose 64 rows lie beyond M stages, waits at the barriers and computes
//   nothing.  No kernel value and no W entry passes through LDS or HBM.
// Staging: points through ko_stage_points in tiles of kKoTJ = 128; V s-major, vs[s][kBwStride] with zeros beyond t and
//   beyond nj.  kBwStride = 160: the 32 lanes of a half wave read 32 consecutive words of row s + h, and rows s, s + 1 lie
//   160 words = 32 banks (mod 64) apart, so the two halves of a wave fall into disjoint halves of 64 banks -- and into all
//   32 banks once each where a half wave is served per pass.  The staging writes run along j: consecutive words too.
// Summation: tile sums added to running sums (two levels), the compensated outputscale sum, block_sum256 and one partial
//   per workgroup; a per-row store for the points.  No atomics, no workgroup waits for another: two calls give equal bits.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using bw_f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kBwStride = kKoTJ + 32;  // words between two columns s of the V tile (see above)

// grid (row blocks, B, js).  POINTS false: part [B, nblk = gridDim.x * gridDim.z, DP + 1], the partials of k_kernel_bil;
// POINTS true: out is g_x1 [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D], as k_kernel_pgrad writes them
template <int FAMILY, int DP, bool POINTS>
__global__ __launch_bounds__(kThreads) void k_kernel_bil_wide(const float* __restrict__ x1, const float* __restrict__ x2,
                                                              const float* __restrict__ theta, int M, int N, int D,
                                                              const float* __restrict__ U, const float* __restrict__ V,
                                                              int t, float* __restrict__ out, int jchunk) {
  constexpr int CH = ko_bil_wide_cols(DP);  // columns s per sweep (even)
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[CH * kBwStride];
  __shared__ float th[DP];
  __shared__ float red[4];
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  const int i = i0 + lane;                                         // the row whose pairs this lane sums
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (i < M && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
    gacc[k] = 0.0f;
  }
  KoKahan gos;  // (the outputscale entry is ONE number per member, a sum of N M terms of both signs)
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
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < 2 * steps * kKoTJ; e += kThreads) {  // (the rows the MFMA steps read, all 128 j)
        const int ss = e / kKoTJ, j = e - ss * kKoTJ;
        vs[ss * kBwStride + j] = (j < nj && s0 + ss < t) ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0f;
      }
      __syncthreads();
      if (i0 >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
      float tacc[DP];         // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int jb = 0; jb < nj; jb += 32) {
        bw_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.0f;
        const float* ap = vs + h * kBwStride + jb + li;
#pragma unroll
        for (int q = 0; q < CH / 2; ++q)
          if (q < steps) {
            const float av = ap[2 * q * kBwStride];
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
          const float* bp = xs + min(j, nj - 1) * DP;
          const float w = j < nj ? wr : 0.0f;
          float sd[DP];
          float r2 = 0.0f;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            sd[k] = a[k] - bp[k];
            r2 = fmaf(sd[k], sd[k], r2);
          }
          float g, hh;
          kf_gh<FAMILY>(r2, &g, &hh);
          const float wh = w * hh;
          if constexpr (POINTS) {
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh, sd[k], tacc[k]);
          } else {
            gos.add(w, g);
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = fmaf(wh * sd[k], sd[k], tacc[k]);
          }
        };
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // ascending j: points 8 q .. 8 q + 3 in acc0, 8 q + 4 .. 8 q + 7 in acc1
#pragma unroll
          for (int m = 0; m < 4; ++m) pair(jb + 8 * q + m, acc0[4 * q + m]);
#pragma unroll
          for (int m = 0; m < 4; ++m) pair(jb + 8 * q + 4 + m, acc1[4 * q + m]);
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  if constexpr (POINTS) {
    if (i < M) {
      const float os2 = theta[b * (D + 1) + D];
      float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
      for (int k = 0; k < DP; ++k)
        if (k < D) o[k] = os2 * th[k] * gacc[k];
    }
  } else {
    const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
    float* o = out + ((size_t)b * nblk + blk) * (DP + 1);
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float sum = block_sum256(gacc[k], red);
      if (threadIdx.x == 0) o[k] = sum;
    }
    const float sum = block_sum256(gos.s, red);
    if (threadIdx.x == 0) o[DP] = sum;
  }
}

template <bool POINTS>
static void bil_wide_launch(const char* name, const KoSweep& w, int family, const float* x1, const float* x2,
                            const float* theta, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                            float* out, hipStream_t st) {
  LO_PROF_BEGIN(name, st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_bil_wide<F(), P(), POINTS>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N,
                       (int)D, U, V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
}

int kernel_bil_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M, int64_t N,
                        int64_t D, const float* U, const float* V, int64_t t, float* g_theta, float* part,
                        hipStream_t st) {
  const KoSweep w(B, M, N, D);
  bil_wide_launch<false>("k_kernel_bil_wide", w, family, x1, x2, theta, M, N, D, U, V, t, part, st);
  LO_LAUNCH_CHECK();
  return ko_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, theta, g_theta, st);
}

int kernel_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                          hipStream_t st) {
  const KoSweep w(B, M, N, D);
  bil_wide_launch<true>("k_kernel_pgrad_wide", w, family, x1, x2, theta, M, N, D, U, V, t, w.s.js > 1 ? part : g_x1, st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko_reduce_splits("k_kernel_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                            LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_bilinear_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_bilinear_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                float* g_theta, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_bil_layout<float>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_bil_wide_run(x1, x2, theta, family, B, M, N, D, U, V, t, g_theta, part, (hipStream_t)stream);
}

size_t lo_kernel_points_grad_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_points_grad_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                   int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                   float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_pgrad_wide_run(x1, x2, theta, family, B, M, N, D, U, V, t, g_x1, part, (hipStream_t)stream);
}

}  // extern "C"
