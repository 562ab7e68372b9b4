// lo_kernel_mv_wide_f64.hip -- the float64 matrix-free kernel product K(x1, x2) v for MANY columns (ABI 44):
// lo_kernel_mv_wide_f64 and the branch of kernel_mv_run_f64 that ko64_wide(c, DP) selects (lo_kernel_shape.h).  K is never
// in memory.
//
// k64_kernel_mv (lo_kernel_op_f64.hip) carries 8 columns of v per sweep (4 at DP = 32) and forms every kernel value -- an
// exp and, for the Matern families, a sqrt of the device math library -- again in the next sweep.  Here the kernel value
// is still formed on the vector ALU, by direct differences in ascending k through kf_g64 (never |a|^2 + |b|^2 - 2 a.b),
// but its product with v runs on v_mfma_f64_16x16x4_f64, so that one value per lane feeds 16 NT columns.
//
// Split of work: a workgroup is 256 threads and owns 256 rows of one member, exactly as k64_kernel_mv (KoSweep, ko_shape,
//   the split-j partials [js, B, M, c] and k64_kernel_mv_reduce are reused unchanged).  A wave owns 64 of those rows as
//   four 16-row tiles, of which it holds R = kw64_rows<DP, NT>() at once (a point costs 2 DP VGPRs, a tile of accumulators
//   16 NT, an exp in flight its temporaries); the remaining row groups run over a restaged tile (one more L2 read of it,
//   small against the exp).  Columns are taken 16 NT per sweep, NT <= 3 (2 at DP = 32: LDS), chosen so that the sweeps are
//   even: 17 columns are one sweep of two tiles, 65 two sweeps of three.
// Operands of D[16 x 16] += A[16 x 4] B[4 x 16] in lane l (li = l % 16, kk = l / 16): A[li][kk], B[kk][li], result register
//   r of 4 is D[4 r + kk][li] (lo_precond.hip, probed: tools/probe/mfma_f64_layout.hip).  Rows are i, the contraction index
//   is j (four points per instruction), the output columns are columns of v.  So lane l keeps the scaled points of its rows
//   ig + 16 t + li, reads the scaled point j + kk of the LDS tile xs once for all R row tiles (4 addresses per wave, each
//   a broadcast within 16 lanes), forms r^2 and g(r) -- its A operands -- and reads its B operands
//   vs[(j + kk) * 16 NT + 16 n + li] (16 consecutive doubles per quarter wave), shared by the R row tiles.  No kernel
//   value passes through LDS or HBM.
// Staging: tiles of kKoTJ = 128 points through ko_stage_points (scaled by theta read from memory: the LDS of a workgroup is
//   xs and vs and nothing else, 64 KB at most); v as [128][16 NT] with zeros beyond c and beyond nj.  The A operand is
//   selected to 0 for j + kk >= nj as well, so whatever xs holds behind a ragged tile contributes nothing.
// Summation: a tile's 32 steps go into a zeroed accumulator, which is then added to the running one (the two levels of
//   k64_kernel_mv).  No atomics, no workgroup waits for another: two calls give equal bits.
// Epilogue: times os2, then [y +] and + d o v when not split, else the partials and k64_kernel_mv_reduce.  For a fixed
//   accumulator register the 16 lanes of a quarter wave hold consecutive columns of one row.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using kw64_f64x4 = __attribute__((ext_vector_type(4))) double;

// row tiles of 16 a wave holds at once: min(4, 16 / DP, 4 / NT), at least one.  A row tile is 2 DP VGPRs of point, 16 NT of
// running and tile sums and one exp of the math library in flight; with min(4, 32 / DP, 8 / NT) seven of the eleven
// (DP, NT) pairs spilled at the 256 registers of two waves per SIMD (48 - 352 bytes of scratch per lane), with this rule none
template <int DP, int NT>
constexpr int kw64_rows() {
  int r = DP <= 4 ? 4 : (DP <= 8 ? 2 : 1);
  if (r * NT > 4) r = NT <= 2 ? 2 : 1;
  return r;
}

// grid (row blocks, B, js); part == nullptr: y is written ([y +] K v + d o v), else the partial products [js, B, M, c]
template <int FAMILY, int DP, int NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k64_kernel_mv_wide(
    const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ theta, int M, int N, int D,
    const double* __restrict__ v, int c, const double* __restrict__ dd_ptr, int dd_mode, int accumulate,
    double* __restrict__ y, double* __restrict__ part, int jchunk) {
  constexpr int R = kw64_rows<DP, NT>(), W = 16 * NT;
  static_assert((kKoTJ * (DP + W)) * sizeof(double) <= 65536, "xs and vs are the workgroup's LDS: 64 KB");
  __shared__ __align__(16) double xs[kKoTJ * DP];
  __shared__ __align__(16) double vs[kKoTJ * W];
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63, li = lane & 15, kk = lane >> 4;
  const int iw = blockIdx.x * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  const double* th = theta + b * (D + 1);
  const double os2 = th[D];
  const double* x2b = x2 + (size_t)b * N * D;
  const double* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += W) {
    for (int g = 0; g < 4 / R; ++g) {
      if ((int)(blockIdx.x * kThreads) + 16 * R * g >= M) break;  // (workgroup uniform: no wave has rows from here on)
      const int ig = iw + 16 * R * g;  // the first row of the wave's group (wave uniform)
      double a[R][DP];
#pragma unroll
      for (int t = 0; t < R; ++t) {
        const int i = ig + 16 * t + li;
#pragma unroll
        for (int k = 0; k < DP; ++k) a[t][k] = (i < M && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0;
      }
      kw64_f64x4 acc[R][NT];
#pragma unroll
      for (int t = 0; t < R; ++t)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = kw64_f64x4{0.0, 0.0, 0.0, 0.0};
      for (int jt = j0; jt < j1; jt += kKoTJ) {
        const int nj = min(kKoTJ, j1 - jt);
        __syncthreads();  // (the previous tile has been read)
        ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
        for (int e = threadIdx.x; e < kKoTJ * W; e += kThreads) {  // (runs of min(W, c - c0) doubles of a row of v)
          const int j = e / W, cc = e - j * W;
          vs[e] = (j < nj && c0 + cc < c) ? vb[(size_t)(jt + j) * c + c0 + cc] : 0.0;
        }
        __syncthreads();
        if (ig >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
        kw64_f64x4 tacc[R][NT];
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
          for (int n = 0; n < NT; ++n) tacc[t][n] = kw64_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < nj; j += 4) {  // (a ragged last step: its points j + kk >= nj are <= 127, masked below)
          const int jj = j + kk;
          const double* bp = xs + jj * DP;
          double r2[R];
#pragma unroll
          for (int t = 0; t < R; ++t) r2[t] = 0.0;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            const double bk = bp[k];
#pragma unroll
            for (int t = 0; t < R; ++t) {
              const double df = a[t][k] - bk;
              r2[t] = fma(df, df, r2[t]);
            }
          }
          double bv[NT];
#pragma unroll
          for (int n = 0; n < NT; ++n) bv[n] = vs[jj * W + 16 * n + li];
#pragma unroll
          for (int t = 0; t < R; ++t) {
            const double kv = jj < nj ? kf_g64<FAMILY>(r2[t]) : 0.0;
#pragma unroll
            for (int n = 0; n < NT; ++n) tacc[t][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, bv[n], tacc[t][n], 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < R; ++t)
#pragma unroll
          for (int n = 0; n < NT; ++n) acc[t][n] += tacc[t][n];
      }
      // accumulator register r of tile (t, n) is row ig + 16 t + 4 r + kk at column c0 + 16 n + li
#pragma unroll
      for (int t = 0; t < R; ++t) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = ig + 16 * t + 4 * r + kk, col = c0 + 16 * n + li;
            if (i < M && col < c) {
              const size_t o = ((size_t)b * M + i) * c + col;
              double res = os2 * acc[t][n][r];
              if (part) {
                part[(size_t)blockIdx.z * gridDim.y * M * c + o] = res;
              } else {
                if (accumulate) res = y[o] + res;
                if (dd_mode == LO_DIAG_FULL) res = fma(dd_ptr[(size_t)b * M + i], v[o], res);
                else if (dd_mode == LO_DIAG_CONST) res = fma(dd_ptr[b], v[o], res);
                y[o] = res;
              }
            }
          }
        }
      }
    }
  }
}

int kernel_mv_wide_run_f64(const double* x1, const double* x2, const double* theta, int family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const double* v, int64_t c, const double* d, int dmode, int accumulate,
                           double* y, double* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  const int NT = ko64_wide_tiles(c, w.DP);
  double* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k64_kernel_mv_wide", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {  // (the tile counts depend on the padded dimension)
    ko_pick(ko64_wide_nts<P()>{}, NT, [&](auto T) {
      hipLaunchKernelGGL((k64_kernel_mv_wide<F(), P(), T()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N,
                         (int)D, v, (int)c, d, dmode, accumulate, y, p, w.s.jchunk);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko64_reduce_splits("k64_kernel_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode,
                              accumulate, v, y, st);
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_mv_wide_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { kernel_mv_layout_f64(ar, B, M, N, c); });
}

int lo_kernel_mv_wide_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const double* v, int64_t c, const double* d, int32_t diag_mode, double* y,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || v == y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = kernel_mv_layout_f64(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_mv_wide_run_f64(x1, x2, theta, family, B, M, N, D, v, c, d, diag_mode, 0, y, part, (hipStream_t)stream);
}

}  // extern "C"
