// lo_kernel_kinds_wide.hip -- the many-column product K(x1, x2) v of the matrix-free kinds with a pair value of their own
// (ABI 46): rational quadratic and periodic (LO_OP_KERNEL_PARAM_DIAG, lo_kernel_param.hip) and spectral mixture
// (LO_OP_KERNEL_SM_DIAG, lo_kernel_sm.hip).  lo_kernel_param_mv_wide_f32, lo_kernel_sm_mv_wide_f32 and the branches of
// kernel_param_mv_run / kernel_sm_mv_run that kp_wide / ksm_wide select (lo_kernel_shape.h).  K is never in memory.
//
// k_kparam_mv and k_ksm_mv form a kernel value -- a logarithm and an exponential, D sines and an exponential, or Q D
// cosines and Q exponentials -- and spend one FMA per column on it, 16 columns per sweep; the next sweep forms every value
// again.  Here the value is formed ONCE per 32 columns, by the device functions and in the operation order of those
// kernels, and its product with v runs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation).
//
// The frame is k_kernel_mv_wide's (lo_kernel_mv_wide.hip), one body for the three families:
//   split      256 threads own 256 rows of one member (KoSweep, ko_shape, the split-j partials [js, B, M, c] and
//              ko_reduce_splits, unchanged); a wave owns 64 rows as two 32-row tiles; 32 columns per sweep, the last ragged
//   operands   lane l (li = l % 32, h = l / 32): A[li][h], B[h][li], accumulator register r of 16 is
//              D[8 (r / 4) + 4 h + r % 4][li].  Rows are i, the contraction index is j (two points per instruction).  The
//              lane keeps the points of its rows i0 + li and i0 + 32 + li in DP registers each, reads point j + h of the
//              LDS tile (one address per half wave: a broadcast that serves both row tiles), forms its two kernel values
//              -- the A operands -- and reads vs[(j + h) * 32 + li], the B operand of both instructions
//   staging    tiles of kKoTJ = 128 points, v as [128][32] with zeros beyond c and beyond nj; the A operand is SELECTED to
//              0 for j >= nj, so whatever xs holds behind a ragged tile contributes nothing
//   summation  a tile's 64 steps go into a zeroed accumulator, which is then added to the running one.  No atomics, no
//              workgroup waits for another: two calls give equal bits
//   epilogue   one 64-bit offset per lane and offsets kr c that are the same for every lane (section 6x says why)
// What differs per family is a value policy (below): what of theta sits in LDS, how a point is staged, the pair value.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using kkw_f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kKkwCols = 32;  // columns of v per sweep: the N of the 32 x 32 x 2 instruction
constexpr int kKkwRT = 2;     // 32-row tiles of a wave

// Rational quadratic and periodic.  LDS: th[DP] = t_k, sc[DP] = what the points are scaled by (RQ: t_k, PERIODIC: nu_k).
//   RQ        r^2 by direct differences of the scaled points in ascending coordinate, kp_rq_g(r^2, alpha, 1 / (2 alpha))
//   PERIODIC  rho = sum_k (t_k sin(pi |a_k - b_k|))^2 in ascending coordinate, kp_per_g(rho)
template <int FAMILY, int DP_>
struct KkwParam {
  static constexpr int DP = DP_;
  static constexpr int kWords = 2 * DP;
  static constexpr bool kOs2 = true;  // the epilogue multiplies by os2
  float *th, *sc;
  float alpha, inv2a;  // (RQ only; PERIODIC never reads them)

  // the member's theta into `tl` (ends with a barrier); returns os2
  __device__ __forceinline__ float load(const float* __restrict__ theta, int64_t b, int D, int, float* tl) {
    const float* tb = theta + b * (2 * D + 2);
    th = tl;
    sc = tl + DP;
    kp_load_theta<FAMILY, DP>(tb, D, th, sc);
    alpha = tb[D + 1];
    inv2a = 0.5f / alpha;
    return tb[D];
  }
  __device__ __forceinline__ float point(float x, int k) const { return x * sc[k]; }
  __device__ __forceinline__ void stage(const float* __restrict__ x2b, int D, int jt, int nj, float* xs) const {
    ko_stage_points<DP>(x2b, sc, D, jt, nj, xs);
  }
  // the values of the rows a[0], a[1] against the staged point bp (each coordinate of bp read once for both)
  __device__ __forceinline__ void values(const float (&a)[kKkwRT][DP], const float* __restrict__ bp,
                                         float (&kv)[kKkwRT]) const {
    float sum[kKkwRT] = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float bk = bp[k];
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t) {
        const float df = a[t][k] - bk;
        if constexpr (FAMILY == LO_KERNEL_PERIODIC) {
          const float ts = th[k] * kp_sinpi(fabsf(df));
          sum[t] = fmaf(ts, ts, sum[t]);
        } else {
          sum[t] = fmaf(df, df, sum[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kKkwRT; ++t)
      kv[t] = FAMILY == LO_KERNEL_PERIODIC ? kp_per_g(sum[t]) : kp_rq_g(sum[t], alpha, inv2a);
  }
};

// Spectral mixture.  LDS as ksm_load_theta lays it out: tmu[Q][DP] = |mu|, tsg[Q][DP] = sigma, tw[Q]; the points stay raw.
// tau_k = |a_k - b_k| once per row tile, then per mixture sum_k (sigma_k tau_k)^2, the product of the cosines in ascending
// coordinate, and kv = fma(w_q, E_q prod, kv) in ascending q: the order of k_ksm_mv.  No os2.
template <int DP_>
struct KkwSm {
  static constexpr int DP = DP_;
  static constexpr int kWords = 2 * kKsmQ * DP + kKsmQ;
  static constexpr bool kOs2 = false;
  float *tmu, *tsg, *tw;
  int Q;

  __device__ __forceinline__ float load(const float* __restrict__ theta, int64_t b, int D, int Q_, float* tl) {
    Q = Q_;
    tmu = tl;
    tsg = tl + kKsmQ * DP;
    tw = tl + 2 * kKsmQ * DP;
    ksm_load_theta<DP>(theta + b * Q * (2 * D + 1), D, Q, tw, tmu, tsg);
    return 1.0f;
  }
  __device__ __forceinline__ float point(float x, int) const { return x; }
  __device__ __forceinline__ void stage(const float* __restrict__ x2b, int D, int jt, int nj, float* xs) const {
    ksm_stage_points<DP>(x2b, D, jt, nj, xs);
  }
  __device__ __forceinline__ void values(const float (&a)[kKkwRT][DP], const float* __restrict__ bp,
                                         float (&kv)[kKkwRT]) const {
    float tau[kKkwRT][DP];
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      const float bk = bp[k];
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t) tau[t][k] = fabsf(a[t][k] - bk);
    }
#pragma unroll
    for (int t = 0; t < kKkwRT; ++t) kv[t] = 0.0f;
    for (int q = 0; q < Q; ++q) {
      float s2[kKkwRT] = {0.0f, 0.0f}, pr[kKkwRT] = {1.0f, 1.0f};
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const float sg = tsg[q * DP + k], mu = tmu[q * DP + k];  // (uniform: a broadcast)
#pragma unroll
        for (int t = 0; t < kKkwRT; ++t) {
          const float st = sg * tau[t][k];
          s2[t] = fmaf(st, st, s2[t]);
          pr[t] *= ksm_cos2pi(mu * tau[t][k]);
        }
      }
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t) kv[t] = fmaf(tw[q], ksm_env(s2[t]) * pr[t], kv[t]);
    }
  }
};

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c].
// Q: the mixtures of the spectral mixture kind (the other policies ignore it).
template <class POL>
__global__ __launch_bounds__(kThreads) void k_kinds_mv_wide(const float* __restrict__ x1, const float* __restrict__ x2,
                                                            const float* __restrict__ theta, int Q, int M, int N, int D,
                                                            const float* __restrict__ v, int c,
                                                            const float* __restrict__ dd_ptr, int dd_mode,
                                                            float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                            const int* __restrict__ stop) {
  constexpr int DP = POL::DP;
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKkwCols];
  __shared__ __align__(16) float tl[POL::kWords];
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  POL pol;
  const float os2 = pol.load(theta, b, D, Q, tl);
  float a[kKkwRT][DP];
#pragma unroll
  for (int t = 0; t < kKkwRT; ++t) {
    const int i = i0 + 32 * t + li;
#pragma unroll
    for (int k = 0; k < DP; ++k) a[t][k] = (i < M && k < D) ? pol.point(x1[((size_t)b * M + i) * D + k], k) : 0.0f;
  }
  const float* x2b = x2 + (size_t)b * N * D;
  const float* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += kKkwCols) {
    kkw_f32x16 acc[kKkwRT];
#pragma unroll
    for (int t = 0; t < kKkwRT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      pol.stage(x2b, D, jt, nj, xs);
      for (int j = threadIdx.x >> 5; j < kKoTJ; j += kThreads / kKkwCols)  // (a row of vs per half wave: runs of <= 32 floats)
        vs[j * kKkwCols + li] = (j < nj && c0 + li < c) ? vb[(size_t)(jt + j) * c + c0 + li] : 0.0f;
      __syncthreads();
      if (i0 >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
      kkw_f32x16 tacc[kKkwRT];
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tacc[t][r] = 0.0f;
      for (int j = 0; j < nj; j += 2) {  // (nj odd: the last step's upper half is j == nj <= 127, masked below)
        const int jj = j + h;
        float kv[kKkwRT];
        pol.values(a, xs + jj * DP, kv);
        const float bv = vs[jj * kKkwCols + li];
#pragma unroll
        for (int t = 0; t < kKkwRT; ++t)
          tacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(jj < nj ? kv[t] : 0.0f, bv, tacc[t], 0, 0, 0);
      }
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t) acc[t] += tacc[t];
    }
    // accumulator register r of tile t is row i0 + 4 h + kr, kr = 32 t + 8 (r / 4) + r % 4 (a constant per register), at
    // column c0 + li: one 64-bit offset per lane, and offsets kr c that are the same for every lane
    if (c0 + li < c) {
      const int ib = i0 + 4 * h;
      const size_t ob = ((size_t)b * M + ib) * c + c0 + li;
      float* out = part ? part + (size_t)blockIdx.z * gridDim.y * M * c + ob : y + ob;
      const int mode = part ? LO_DIAG_NONE : dd_mode;
      const float* vrow = v + ob;
      const float* drow = dd_ptr + (mode == LO_DIAG_FULL ? (size_t)b * M + ib : (size_t)0);
      const float dconst = mode == LO_DIAG_CONST ? dd_ptr[b] : 0.0f;
#pragma unroll
      for (int t = 0; t < kKkwRT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = 32 * t + 8 * (r >> 2) + (r & 3);
          if (ib + kr < M) {
            float res = POL::kOs2 ? os2 * acc[t][r] : acc[t][r];
            if (mode == LO_DIAG_FULL) res = fmaf(drow[kr], vrow[(size_t)kr * c], res);
            else if (mode == LO_DIAG_CONST) res = fmaf(dconst, vrow[(size_t)kr * c], res);
            out[(size_t)kr * c] = res;
          }
        }
      }
    }
  }
}

// the launch both kinds share: `launch(grid, part or nullptr, jchunk, dmode)` starts the family's instantiation
template <class L>
static int kkw_run(const char* reduce_name, int64_t B, int64_t M, int64_t N, int64_t D, const float* v, int64_t c,
                   const float* d, int dmode, float* y, float* part, const int* stop, hipStream_t st, L&& launch) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_kinds_mv_wide", st);
  launch(w, p, dmode);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits(reduce_name, p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y, stop, st);
  return LO_OK;
}

int kernel_param_mv_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                             int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y,
                             float* part, const int* stop, hipStream_t st) {
  return kkw_run("k_kparam_mv_wide_reduce", B, M, N, D, v, c, d, dmode, y, part, stop, st,
                 [&](const KoSweep& w, float* p, int mode) {
                   kp_dispatch(family, w.DP, [&](auto F, auto P) {
                     hipLaunchKernelGGL((k_kinds_mv_wide<KkwParam<F(), P()>>), w.grid, dim3(kThreads), 0, st, x1, x2, theta,
                                        0, (int)M, (int)N, (int)D, v, (int)c, d, mode, y, p, w.s.jchunk, stop);
                   });
                 });
}

int kernel_sm_mv_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                          int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                          const int* stop, hipStream_t st) {
  return kkw_run("k_ksm_mv_wide_reduce", B, M, N, D, v, c, d, dmode, y, part, stop, st,
                 [&](const KoSweep& w, float* p, int mode) {
                   ko_pick(ksm_dims{}, w.DP, [&](auto P) {
                     hipLaunchKernelGGL((k_kinds_mv_wide<KkwSm<P()>>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, Q,
                                        (int)M, (int)N, (int)D, v, (int)c, d, mode, y, p, w.s.jchunk, stop);
                   });
                 });
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_param_mv_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !kp_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_param_mv_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B,
                                int64_t M, int64_t N, int64_t D, const float* v, int64_t c, const float* d,
                                int32_t diag_mode, float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c) || !kp_family_ok(family)) return LO_ERR_BADARG;
  if (!kp_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!kp_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_param_mv_wide_run(x1, x2, theta, family, B, M, N, D, v, c, d, diag_mode, y, part, nullptr,
                                  (hipStream_t)stream);
}

size_t lo_kernel_sm_mv_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  if (!ksm_args_ok(B, M, N, D, Q, c) || !ksm_shape_ok(B, M, N, D, Q, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_sm_mv_wide_f32(const float* x1, const float* x2, const float* theta, int32_t Q, int64_t B, int64_t M,
                             int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                             void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ksm_args_ok(B, M, N, D, Q, c)) return LO_ERR_BADARG;
  if (!ksm_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ksm_shape_ok(B, M, N, D, Q, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_sm_mv_wide_run(x1, x2, theta, Q, B, M, N, D, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

}  // extern "C"
