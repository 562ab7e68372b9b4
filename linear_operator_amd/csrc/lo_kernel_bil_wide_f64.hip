// lo_kernel_bil_wide_f64.hip -- the float64 derivatives of sum_s u_s^T K(x1, x2) v_s for MANY columns s (ABI 45):
// lo_kernel_bilinear_wide_f64, lo_kernel_points_grad_wide_f64 and the branch of kernel_bil_run_f64 / kernel_pgrad_run_f64
// that ko64_bil_wide selects (lo_kernel_shape.h).  K is never in memory.
//
// k64_kernel_bil and k64_kernel_pgrad (lo_kernel_op_f64.hip) form W_ij = sum_s U_is V_js with ko64_ts(DP) = 8 / 4 / 2 vector
// FMAs per pair and form every r^2, the math library's exp and sqrt and the scaled differences again in the next sweep.
// Here W = U V^T, a GEMM with contraction length t, runs on v_mfma_f64_16x16x4_f64, up to ko64_bil_wide_cols(DP) columns
// per sweep, and the pair work happens once per pair and sweep.
//
// Split of work: that of k64_kernel_bil / k64_kernel_pgrad.  A workgroup is 256 threads and owns 256 rows of one member
//   (KoSweep, ko_shape, split-j over gridDim.z; ko_bil_layout<double> / k64_kernel_bil_reduce for the hyperparameters,
//   ko_split_layout<double> / ko64_reduce_splits for the points).  A wave owns 64 rows as four 16-row tiles tau = 0 .. 3.
// W on the matrix cores, transposed: per block of 16 points j of the LDS tile and per row tile,
//   W^T[16 j x 16 i] += V^T[16 j x 4 s] U^T[4 s x 16 i].  Operands of D[16 x 16] += A[16 x 4] B[4 x 16] in lane l
//   (li = l % 16, kk = l / 16): A[li][kk], B[kk][li], result register r of 4 is D[4 r + kk][li] (lo_kernel_mv_wide_f64.hip,
//   probed: tools/probe/mfma_f64_layout.hip).  So the A operand is V[jb + li][s + kk], read from LDS and shared by the four
//   row tiles; the B operand is U[iw + 16 tau + li][s + kk], kept in registers for the whole sweep; ceil(cols / 4) steps for
//   the sweep's actual column count, a wave-uniform bound.  Result register r of tile tau is W[iw + 16 tau + li][jb + 4 r + kk].
// One row per lane again: the tile index tau (a register index) and the point sub-index kk (a 16-lane group) are exchanged,
//   a 4 x 4 transpose between registers and 16-lane groups, in two steps per 32-bit half of a double.  With tau = 2 t1 + t0
//   and kk = 2 k1 + k0: v_permlane32_swap_b32 on the register pairs (tau, tau + 2) exchanges lanes 32 - 63 of its first operand
//   with lanes 0 - 31 of its second, i.e. t1 with k1; v_permlane16_swap_b32 on the pairs (tau, tau + 1), tau even, exchanges
//   the odd 16-lane rows of its first operand with the even rows of its second, i.e. t0 with k0.  Afterwards lane l owns
//   row iw + l -- the row mapping of the plain kernels -- and in every lane register (m, r) is point jb + 4 r + m: 32 swaps
//   per 1024 pairs.  So the lane keeps ONE scaled point a[DP], and every read of the point tile xs is one wave-uniform
//   address.
// Pair loop: the inner loop of the plain kernels with w taken from a transposed accumulator register, the 16 points of a
//   block in ascending j, r^2 by direct differences in ascending k, kf_gh64 unchanged, the scaled differences formed twice.
//   For j >= nj of a ragged block of 16 the point read is the tile's last valid one (a wave-uniform clamp of the index, so
//   nothing that xs holds behind the end is ever read) and w is SELECTED to 0, not multiplied.  Rows beyond M carry zero
//   U, so they add nothing and store nothing; a wave whose 64 rows lie beyond M stages, waits at the barriers and computes
//   nothing.  No kernel value and no W entry passes through LDS or HBM.
// Staging: points through ko_stage_points in tiles of kKoTJ = 128; V s-major, vs[s][kBw64Stride] with zeros beyond t and
//   beyond nj, only the 4 * steps rows the MFMA steps read.  kBw64Stride = 144 doubles: the 16 lanes of a quarter wave read
//   16 consecutive doubles (32 consecutive banks of 4 bytes) of row s + kk at word address 2 ((s + kk) 144 + jb + li), and
//   two neighbouring rows lie 288 words = 32 banks (mod 64) apart, so the two quarter waves a 64-bit read serves per pass
//   (kk = 0, 1, then kk = 2, 3) fall into disjoint halves of the 64 banks.  The staging writes run along j: consecutive
//   doubles too.  xs and vs are DP + 1.125 cols KB: 64 KB of static LDS bound the columns at DP 4, 8 and 32 (lo_kernel_shape.h).
// Summation: tile sums added to running sums (two levels), the compensated outputscale sum, block_sum256_d and one partial
//   per workgroup; a per-row store for the points.  No atomics, no workgroup waits for another: two calls give equal bits.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using bw64_f64x4 = __attribute__((ext_vector_type(4))) double;
constexpr int kBw64Stride = kKoTJ + 16;  // doubles between two columns s of the V tile (see above)

// x, y: one register each of two tiles.  SWAP32: lanes 32 - 63 of x <-> lanes 0 - 31 of y; else the odd 16-lane rows of x
// <-> the even rows of y.  Both 32-bit halves of the doubles move alike.
template <bool SWAP32>
__device__ __forceinline__ void bw64_swap(double& x, double& y) {
  const unsigned long long ux = __double_as_longlong(x), uy = __double_as_longlong(y);
  unsigned lo[2], hi[2];
  if constexpr (SWAP32) {
    const auto l = __builtin_amdgcn_permlane32_swap((unsigned)ux, (unsigned)uy, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap((unsigned)(ux >> 32), (unsigned)(uy >> 32), false, false);
    lo[0] = l[0], lo[1] = l[1], hi[0] = h[0], hi[1] = h[1];
  } else {
    const auto l = __builtin_amdgcn_permlane16_swap((unsigned)ux, (unsigned)uy, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((unsigned)(ux >> 32), (unsigned)(uy >> 32), false, false);
    lo[0] = l[0], lo[1] = l[1], hi[0] = h[0], hi[1] = h[1];
  }
  x = __longlong_as_double(((unsigned long long)hi[0] << 32) | lo[0]);
  y = __longlong_as_double(((unsigned long long)hi[1] << 32) | lo[1]);
}

// grid (row blocks, B, js).  POINTS false: out is part [B, nblk = gridDim.x * gridDim.z, DP + 1], the partials of
// k64_kernel_bil; POINTS true: out is g_x1 [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D], as
// k64_kernel_pgrad writes them
template <int FAMILY, int DP, bool POINTS>
__global__ __launch_bounds__(kThreads, ko64_waves<DP>()) void k64_kernel_bil_wide(
    const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ theta, int M, int N, int D,
    const double* __restrict__ U, const double* __restrict__ V, int t, double* __restrict__ out, int jchunk) {
  constexpr int CH = ko64_bil_wide_cols(DP);  // columns s per sweep (a multiple of 4)
  constexpr int QS = CH / 4;                  // contraction steps of a full sweep
  static_assert(CH % 4 == 0, "a contraction step is four columns");
  static_assert((kKoTJ * DP + CH * kBw64Stride + DP + 4) * sizeof(double) <= 65536, "static LDS: 64 KB");
  __shared__ __align__(16) double xs[kKoTJ * DP];
  __shared__ __align__(16) double vs[CH * kBw64Stride];
  __shared__ double th[DP];
  __shared__ double red[4];
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63, li = lane & 15, kk = lane >> 4;
  const int iw = blockIdx.x * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  const int i = iw + lane;                                         // the row whose pairs this lane sums
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0;
  __syncthreads();
  double a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (i < M && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0;
    gacc[k] = 0.0;
  }
  double gos = 0.0, gos_c = 0.0;  // (the outputscale entry is ONE number per member: compensated, as in k64_kernel_bil)
  const double* x2b = x2 + (size_t)b * N * D;
  const double* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += CH) {
    const int steps = (min(CH, t - s0) + 3) / 4;  // contraction steps of this sweep: four columns each
    double ub[4][QS];                             // the B operands: U[iw + 16 tau + li][s0 + 4 q + kk]
#pragma unroll
    for (int tau = 0; tau < 4; ++tau) {
      const int iu = iw + 16 * tau + li;
#pragma unroll
      for (int q = 0; q < QS; ++q) {
        const int s = s0 + 4 * q + kk;
        ub[tau][q] = (iu < M && s < t) ? U[((size_t)b * M + iu) * t + s] : 0.0;
      }
    }
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < 4 * steps * kKoTJ; e += kThreads) {  // (the rows the MFMA steps read, all 128 j)
        const int ss = e / kKoTJ, j = e - ss * kKoTJ;
        vs[ss * kBw64Stride + j] = (j < nj && s0 + ss < t) ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0;
      }
      __syncthreads();
      if (iw >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
      double tacc[DP];        // (a tile's sums on their own, then added to the running ones, as in the plain kernels)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0;
      for (int jb = 0; jb < nj; jb += 16) {
        bw64_f64x4 acc[4];
#pragma unroll
        for (int tau = 0; tau < 4; ++tau) acc[tau] = bw64_f64x4{0.0, 0.0, 0.0, 0.0};
        const double* ap = vs + kk * kBw64Stride + jb + li;
#pragma unroll
        for (int q = 0; q < QS; ++q)
          if (q < steps) {
            const double av = ap[4 * q * kBw64Stride];
#pragma unroll
            for (int tau = 0; tau < 4; ++tau)
              acc[tau] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, ub[tau][q], acc[tau], 0, 0, 0);
          }
        // register r of tile tau in lane group kk (row 16 tau + li, point 4 r + kk) -> register r of "tile" m in lane
        // group kk: row 16 kk + li, point 4 r + m
        double wt[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int tau = 0; tau < 4; ++tau) wt[tau][r] = acc[tau][r];
          bw64_swap<true>(wt[0][r], wt[2][r]);
          bw64_swap<true>(wt[1][r], wt[3][r]);
          bw64_swap<false>(wt[0][r], wt[1][r]);
          bw64_swap<false>(wt[2][r], wt[3][r]);
        }
        auto pair = [&](int j, double wr) {  // j: wave uniform
          const double* bp = xs + min(j, nj - 1) * DP;
          const double w = j < nj ? wr : 0.0;
          double r2 = 0.0;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            const double df = a[k] - bp[k];
            r2 = fma(df, df, r2);
          }
          double g, h;
          kf_gh64<FAMILY>(r2, &g, &h);
          const double wh = w * h;
          if constexpr (POINTS) {
#pragma unroll
            for (int k = 0; k < DP; ++k) tacc[k] = fma(wh, a[k] - bp[k], tacc[k]);
          } else {
            const double term = fma(w, g, -gos_c);
            const double next = gos + term;
            gos_c = (next - gos) - term;
            gos = next;
#pragma unroll
            for (int k = 0; k < DP; ++k) {
              const double df = a[k] - bp[k];
              tacc[k] = fma(wh * df, df, tacc[k]);
            }
          }
        };
        // Ascending j = jb + 4 r + m in rolled loops: 16 unrolled pairs let the exps of all of them overlap, which costs up
        // to 3.5 KB of scratch per lane.  A trip takes the four points of one r from register 0 of every m, then the
        // registers move down; Matern-1/2, whose h holds a division, takes ONE point per trip from register (0, 0) and
        // rotates the four m (four trips put them back)
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          if constexpr (FAMILY == LO_KERNEL_MATERN12) {
#pragma unroll 1
            for (int m = 0; m < 4; ++m) {
              pair(jb + 4 * r + m, wt[0][0]);
              const double first = wt[0][0];
              wt[0][0] = wt[1][0], wt[1][0] = wt[2][0], wt[2][0] = wt[3][0], wt[3][0] = first;
            }
          } else {
#pragma unroll
            for (int m = 0; m < 4; ++m) pair(jb + 4 * r + m, wt[m][0]);
          }
#pragma unroll
          for (int m = 0; m < 4; ++m) wt[m][0] = wt[m][1], wt[m][1] = wt[m][2], wt[m][2] = wt[m][3];
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  if constexpr (POINTS) {
    if (i < M) {
      const double os2 = theta[b * (D + 1) + D];
      double* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
      for (int k = 0; k < DP; ++k)
        if (k < D) o[k] = os2 * th[k] * gacc[k];
    }
  } else {
    const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
    double* o = out + ((size_t)b * nblk + blk) * (DP + 1);
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const double sum = block_sum256_d(gacc[k], red);
      if (threadIdx.x == 0) o[k] = sum;
    }
    const double sum = block_sum256_d(gos, red);
    if (threadIdx.x == 0) o[DP] = sum;
  }
}

template <bool POINTS>
static void bil_wide_launch_f64(const char* name, const KoSweep& w, int family, const double* x1, const double* x2,
                                const double* theta, int64_t M, int64_t N, int64_t D, const double* U, const double* V,
                                int64_t t, double* out, hipStream_t st) {
  LO_PROF_BEGIN(name, st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k64_kernel_bil_wide<F(), P(), POINTS>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M,
                       (int)N, (int)D, U, V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
}

int kernel_bil_wide_run_f64(const double* x1, const double* x2, const double* theta, int family, int64_t B, int64_t M,
                            int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_theta,
                            double* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  bil_wide_launch_f64<false>("k64_kernel_bil_wide", w, family, x1, x2, theta, M, N, D, U, V, t, part, st);
  LO_LAUNCH_CHECK();
  return ko64_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, theta, g_theta, st);
}

int kernel_pgrad_wide_run_f64(const double* x1, const double* x2, const double* theta, int family, int64_t B, int64_t M,
                              int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_x1,
                              double* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  bil_wide_launch_f64<true>("k64_kernel_pgrad_wide", w, family, x1, x2, theta, M, N, D, U, V, t,
                            w.s.js > 1 ? part : g_x1, st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko64_reduce_splits("k64_kernel_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                              LO_DIAG_NONE, 0, nullptr, g_x1, st);
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_bilinear_wide_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<double>(ar, B, M, N, D); });
}

int lo_kernel_bilinear_wide_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B,
                                int64_t M, int64_t N, int64_t D, const double* U, const double* V, int64_t t,
                                double* g_theta, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = ko_bil_layout<double>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_bil_wide_run_f64(x1, x2, theta, family, B, M, N, D, U, V, t, g_theta, part, (hipStream_t)stream);
}

size_t lo_kernel_points_grad_wide_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<double>(ar, B, M, N, D); });
}

int lo_kernel_points_grad_wide_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B,
                                   int64_t M, int64_t N, int64_t D, const double* U, const double* V, int64_t t,
                                   double* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = ko_split_layout<double>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_pgrad_wide_run_f64(x1, x2, theta, family, B, M, N, D, U, V, t, g_x1, part, (hipStream_t)stream);
}

}  // extern "C"
