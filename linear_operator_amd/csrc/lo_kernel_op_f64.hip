// lo_kernel_op_f64.hip -- the float64 twins of the three sweeps of lo_kernel_op.hip (ABI 31): lo_kernel_mv_f64,
// lo_kernel_bilinear_f64, lo_kernel_points_grad_f64 and the kind LO_OP_KERNEL_DIAG of lo_matvec_f64.  A float64
// KernelLinearOperator never forms K either; the fp32 kernels are a file of their own and do not move.
//
// Product (k64_kernel_mv): the structure of k_kernel_mv -- 256 rows per workgroup, one per thread, the scaled point in
//   registers (two VGPRs per coordinate), x2 scaled while it is staged in LDS tiles of 128, r^2 by direct differences in
//   ascending k, a tile's sum formed on its own and then added to the running one, the columns j split over gridDim.z
//   when there are few row blocks (ko_shape), partials in the workspace, k64_kernel_mv_reduce adds them in ascending
//   order and applies + d o v.  exp / sqrt are the device math library's (lo_kernel_fn.h: kf_g64).  `accumulate`: the
//   product is added onto y (a later term of a float64 LO_OP_SUM), in the direct store and in the reduce kernel.
// Derivative (k64_kernel_bil) and points (k64_kernel_pgrad): the sums of k_kernel_bil / k_kernel_pgrad, W_ij formed in
//   chunks of ko64_ts(DP) columns; the scaled differences are formed twice (for r^2, then for the sums) instead of being
//   kept, which is what lets DP = 32 stay in registers.
// No atomics, no workgroup waits for another: two calls give equal bits.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

// (columns of v per sweep: ko64_col_chunk / ko64_cols of lo_kernel_shape.h)

// columns s of U / V per sweep of the derivatives
template <int DP>
constexpr int ko64_ts() {
  return DP <= 8 ? 8 : (DP == 16 ? 4 : 2);
}

// waves per SIMD the derivative kernels are held to (the second argument of __launch_bounds__, i.e. amdgpu_waves_per_eu):
// two (<= 256 VGPRs) up to DP = 16; at DP = 32 the point, the running and the tile sums are 192 VGPRs before anything
// else, so one wave per SIMD, whose budget of 512 lets the accumulation registers hold what does not fit
template <int DP>
constexpr int ko64_waves() {
  return DP == 32 ? 1 : 2;
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

// grid (row blocks, B, js); part == nullptr: y is written ([y +] K v + d o v), else the partial products [js, B, M, c]
template <int FAMILY, int DP, int CC>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k64_kernel_mv(
    const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ theta, int M, int N, int D,
    const double* __restrict__ v, int c, const double* __restrict__ dd_ptr, int dd_mode, int accumulate,
    double* __restrict__ y, double* __restrict__ part, int jchunk) {
  __shared__ __align__(16) double xs[kKoTJ * DP];
  __shared__ __align__(16) double vs[kKoTJ * CC];
  __shared__ double th[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0;
  __syncthreads();
  double a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0;
  const double os2 = theta[b * (D + 1) + D];
  const double* x2b = x2 + (size_t)b * N * D;
  const double* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += CC) {
    double acc[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * CC; e += kThreads) {
        const int j = e / CC, cc = e - j * CC;
        vs[e] = c0 + cc < c ? vb[(size_t)(jt + j) * c + c0 + cc] : 0.0;
      }
      __syncthreads();
      double tacc[CC];
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) tacc[cc] = 0.0;
      for (int j = 0; j < nj; ++j) {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double df = a[k] - xs[j * DP + k];
          r2 = fma(df, df, r2);
        }
        const double kv = kf_g64<FAMILY>(r2);
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) tacc[cc] = fma(kv, vs[j * CC + cc], tacc[cc]);
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
          double r = os2 * acc[cc];
          if (part) {
            part[(size_t)blockIdx.z * gridDim.y * M * c + o] = r;
          } else {
            if (accumulate) r = y[o] + r;
            if (dd_mode == LO_DIAG_FULL) r = fma(dd_ptr[(size_t)b * M + i], v[o], r);
            else if (dd_mode == LO_DIAG_CONST) r = fma(dd_ptr[b], v[o], r);
            y[o] = r;
          }
        }
      }
    }
  }
}

// y[b, i, col] = [y +] sum_z part[z, b, i, col] (ascending z) + d o v; one thread per output element
__global__ __launch_bounds__(kThreads) void k64_kernel_mv_reduce(const double* __restrict__ part, int js,
                                                                 size_t per_member, size_t total, int c,
                                                                 const double* __restrict__ dd_ptr, int dd_mode,
                                                                 int accumulate, const double* __restrict__ v,
                                                                 double* __restrict__ y) {
  const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= total) return;
  double r = part[o];
  for (int z = 1; z < js; ++z) r += part[(size_t)z * total + o];
  if (accumulate) r = y[o] + r;
  if (dd_mode == LO_DIAG_FULL) r = fma(dd_ptr[o / c], v[o], r);
  else if (dd_mode == LO_DIAG_CONST) r = fma(dd_ptr[o / per_member], v[o], r);
  y[o] = r;
}

// grid (row blocks, B, js); part [B, nblk = gridDim.x * gridDim.z, DP + 1]
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads, ko64_waves<DP>()) void k64_kernel_bil(
    const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ theta, int M, int N, int D,
    const double* __restrict__ U, const double* __restrict__ V, int t, double* __restrict__ part, int jchunk) {
  constexpr int TS = ko64_ts<DP>();
  __shared__ __align__(16) double xs[kKoTJ * DP];
  __shared__ __align__(16) double vs[kKoTJ * TS];
  __shared__ double th[DP];
  __shared__ double red[4];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0;
  __syncthreads();
  double a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0;
    gacc[k] = 0.0;
  }
  double gos = 0.0, gos_c = 0.0;
  const double* x2b = x2 + (size_t)b * N * D;
  const double* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += TS) {
    double u[TS];
#pragma unroll
    for (int ss = 0; ss < TS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * TS; e += kThreads) {
        const int j = e / TS, ss = e - j * TS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0;
      }
      __syncthreads();
      double tacc[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0;
      for (int j = 0; j < nj; ++j) {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double df = a[k] - xs[j * DP + k];
          r2 = fma(df, df, r2);
        }
        double g, h;
        kf_gh64<FAMILY>(r2, &g, &h);
        double w = 0.0;
#pragma unroll
        for (int ss = 0; ss < TS; ++ss) w = fma(u[ss], vs[j * TS + ss], w);
        {  // the outputscale entry is ONE number per member, a sum of N M terms of both signs: compensated (Kahan)
          const double term = fma(w, g, -gos_c);
          const double next = gos + term;
          gos_c = (next - gos) - term;
          gos = next;
        }
        const double wh = w * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double df = a[k] - xs[j * DP + k];
          tacc[k] = fma(wh * df, df, tacc[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
  double* out = part + ((size_t)b * nblk + blk) * (DP + 1);
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const double sum = block_sum256_d(gacc[k], red);
    if (threadIdx.x == 0) out[k] = sum;
  }
  const double sum = block_sum256_d(gos, red);
  if (threadIdx.x == 0) out[DP] = sum;
}

// g_theta[b, q] from the nblk partials in ascending order: q < D: os2 / theta[q] times the sum, q == D: the sum
__global__ __launch_bounds__(64) void k64_kernel_bil_reduce(const double* __restrict__ part, int nblk, int DP, int D,
                                                            const double* __restrict__ theta,
                                                            double* __restrict__ g_theta) {
  const int64_t b = blockIdx.x;
  const int q = threadIdx.x;
  if (q > D) return;
  const int slot = q < D ? q : DP;
  const double* p = part + (size_t)b * nblk * (DP + 1) + slot;
  double s = 0.0;
  for (int k = 0; k < nblk; ++k) s += p[(size_t)k * (DP + 1)];
  if (q < D) {
    const double tq = theta[b * (D + 1) + q];
    s = tq != 0.0 ? s * theta[b * (D + 1) + D] / tq : 0.0;
  }
  g_theta[b * (D + 1) + q] = s;
}

// g[b, i, k] = theta_D theta_k sum_j W_ij h(r_ij) s_k, s = theta o (x1_i - x2_j); a thread owns row i.  `out` is g_x1
// [B, M, D] when gridDim.z == 1, else the partials [js, B, M, D] of the column splits (the scale is applied here)
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads, ko64_waves<DP>()) void k64_kernel_pgrad(
    const double* __restrict__ x1, const double* __restrict__ x2, const double* __restrict__ theta, int M, int N, int D,
    const double* __restrict__ U, const double* __restrict__ V, int t, double* __restrict__ out, int jchunk) {
  constexpr int TS = ko64_ts<DP>();
  __shared__ __align__(16) double xs[kKoTJ * DP];
  __shared__ __align__(16) double vs[kKoTJ * TS];
  __shared__ double th[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * (D + 1) + threadIdx.x] : 0.0;
  __syncthreads();
  double a[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0;
    acc[k] = 0.0;
  }
  const double os2 = theta[b * (D + 1) + D];
  const double* x2b = x2 + (size_t)b * N * D;
  const double* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += TS) {
    double u[TS];
#pragma unroll
    for (int ss = 0; ss < TS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int e = threadIdx.x; e < nj * TS; e += kThreads) {
        const int j = e / TS, ss = e - j * TS;
        vs[e] = s0 + ss < t ? Vb[(size_t)(jt + j) * t + s0 + ss] : 0.0;
      }
      __syncthreads();
      double tacc[DP];
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0;
      for (int j = 0; j < nj; ++j) {
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const double df = a[k] - xs[j * DP + k];
          r2 = fma(df, df, r2);
        }
        double g, h;
        kf_gh64<FAMILY>(r2, &g, &h);
        double w = 0.0;
#pragma unroll
        for (int ss = 0; ss < TS; ++ss) w = fma(u[ss], vs[j * TS + ss], w);
        const double wh = w * h;
#pragma unroll
        for (int k = 0; k < DP; ++k) tacc[k] = fma(wh, a[k] - xs[j * DP + k], tacc[k]);
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) acc[k] += tacc[k];
    }
  }
  if (live) {
    double* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = os2 * th[k] * acc[k];
  }
}

static int ko64_reduce_splits(const char* prof_name, const double* part, int js, size_t per_member, size_t total, int c,
                              const double* d, int dmode, int accumulate, const double* v, double* y, hipStream_t st) {
  LO_PROF_BEGIN(prof_name, st);
  hipLaunchKernelGGL(k64_kernel_mv_reduce, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                     part, js, per_member, total, c, d, dmode, accumulate, v, y);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// the product on validated arguments; part: [js, B, M, c] doubles when ko_shape(B, M, N).js > 1 (else unused)
int kernel_mv_run_f64(const double* x1, const double* x2, const double* theta, int family, int64_t B, int64_t M,
                      int64_t N, int64_t D, const double* v, int64_t c, const double* d, int dmode, int accumulate,
                      double* y, double* part, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  const int CC = ko64_col_chunk(c, w.DP);
  double* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k64_kernel_mv", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {  // (the column list depends on the padded dimension)
    ko_pick(ko64_cols<P()>{}, CC, [&](auto C) {
      hipLaunchKernelGGL((k64_kernel_mv<F(), P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N,
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

// the one layout of the product's workspace: the partials of a split member
double* kernel_mv_layout_f64(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t c) {
  return ko_split_layout<double>(ar, B, M, N, c);
}

// LO_OP_KERNEL_DIAG of lo_matvec_f64 (A0 = X, A1 = theta: doubles), validated as the fp32 plan validates it
int kernel_desc_check_f64(const lo_op_desc* op, int64_t c) {
  if (!op->A0 || !op->A1 || op->R < 1 || !ko_family_ok(op->n2)) return LO_ERR_BADARG;
  if (!ko_shape_ok(op->B, op->N, op->N, op->R) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_mv_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { kernel_mv_layout_f64(ar, B, M, N, c); });
}

int lo_kernel_mv_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B, int64_t M,
                     int64_t N, int64_t D, const double* v, int64_t c, const double* d, int32_t diag_mode, double* y,
                     void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || v == y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = kernel_mv_layout_f64(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_mv_run_f64(x1, x2, theta, family, B, M, N, D, v, c, d, diag_mode, 0, y, part, (hipStream_t)stream);
}

size_t lo_kernel_bilinear_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<double>(ar, B, M, N, D); });
}

int lo_kernel_bilinear_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B, int64_t M,
                           int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_theta, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = ko_bil_layout<double>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k64_kernel_bil", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k64_kernel_bil<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D, U,
                       V, (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k64_kernel_bil_reduce, dim3((unsigned)B), dim3(64), 0, st, part, w.s.rb * w.s.js, w.DP, (int)D, theta,
                     g_theta);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

size_t lo_kernel_points_grad_f64_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<double>(ar, B, M, N, D); });
}

int lo_kernel_points_grad_f64(const double* x1, const double* x2, const double* theta, int32_t family, int64_t B,
                              int64_t M, int64_t N, int64_t D, const double* U, const double* V, int64_t t, double* g_x1,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  double* part = ko_split_layout<double>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  double* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k64_kernel_pgrad", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k64_kernel_pgrad<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D,
                       U, V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order (the reduction of the product with D as its columns and no diagonal)
    return ko64_reduce_splits("k64_kernel_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                              LO_DIAG_NONE, 0, nullptr, g_x1, st);
  return LO_OK;
}

}  // extern "C"

