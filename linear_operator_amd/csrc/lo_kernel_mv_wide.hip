// lo_kernel_mv_wide.hip -- the matrix-free kernel product K(x1, x2) v for MANY columns (ABI 42): lo_kernel_mv_wide_f32 and
// the branch of kernel_mv_run that ko_wide(c, DP) selects (lo_kernel_shape.h).  K is never in memory.
//
// k_kernel_mv (lo_kernel_op.hip) spends one vector FMA per kernel value and column, 16 columns per sweep, and forms every
// kernel value again in the next sweep.  Here the kernel value is still formed on the vector ALU, by direct differences
// (never |a|^2 + |b|^2 - 2 a.b), but its product with v runs on v_mfma_f32_32x32x2_f32 -- exact fp32 products, fp32
// accumulation -- so that one value per lane feeds 32 columns in one instruction, beside the ALU work of the other waves.
//
// Split of work: a workgroup is 256 threads and owns 256 rows of one member, exactly as k_kernel_mv (KoSweep, ko_shape, the
//   split-j partials [js, B, M, c] and k_kernel_mv_reduce are reused unchanged).  A wave owns 64 of those rows as two
//   32-row tiles; columns are taken 32 per sweep, the last sweep ragged.
// Operands of D[32 x 32] += A[32 x 2] B[2 x 32] in lane l (li = l % 32, h = l / 32): A[li][h], B[h][li], accumulator
//   register r of 16 is D[8 (r / 4) + 4 h + r % 4][li] (lo_chol.hip mfma_row).  Rows are i, the contraction index is j (two
//   points per instruction), the output columns are the columns of v.  So lane l keeps the scaled points of its rows
//   i0 + li and i0 + 32 + li in DP registers each, reads the scaled point j + h of the LDS tile xs (one address per half
//   wave: a broadcast, and one read serves both row tiles), forms r^2 and g(r) -- its A operands -- and reads its B operand
//   vs[(j + h) * 32 + li] (64 consecutive floats per wave: conflict free), shared by the two MFMAs.  No kernel value passes
//   through LDS or HBM.
// Staging: tiles of kKoTJ = 128 points through ko_stage_points; v as [128][32] with zeros beyond c and beyond nj.  The A
//   operand is selected to 0 for j >= nj as well, so whatever xs holds behind a ragged tile contributes nothing.
// Summation: a tile's 64 steps go into a zeroed accumulator, which is then added to the running one (the two levels of
//   k_kernel_mv).  No atomics, no workgroup waits for another: two calls give equal bits.
// Epilogue: times os2, then + d o v when not split, else the partials and k_kernel_mv_reduce.  For a fixed accumulator
//   register the 32 lanes of a half wave hold consecutive columns of one row: stores are runs of min(32, c - c0) floats.
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

using kw_f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kKwCols = 32;  // columns of v per sweep: the N of the 32 x 32 x 2 instruction

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M, c]
template <int FAMILY, int DP>
__global__ __launch_bounds__(kThreads) void k_kernel_mv_wide(const float* __restrict__ x1, const float* __restrict__ x2,
                                                             const float* __restrict__ theta, int tstride, int M, int N,
                                                             int D, const float* __restrict__ v, int c,
                                                             const float* __restrict__ dd_ptr, int dd_mode,
                                                             float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                             const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * kKwCols];
  __shared__ float th[DP];
  const int64_t b = blockIdx.y;
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const int i0 = blockIdx.x * kThreads + (threadIdx.x >> 6) * 64;  // the wave's first row (wave uniform)
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * tstride + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[2][DP];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int i = i0 + 32 * t + li;
#pragma unroll
    for (int k = 0; k < DP; ++k) a[t][k] = (i < M && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
  }
  const float os2 = theta[b * tstride + D];
  const float* x2b = x2 + (size_t)b * N * D;
  const float* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += kKwCols) {
    kw_f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      ko_stage_points<DP>(x2b, th, D, jt, nj, xs);
      for (int j = threadIdx.x >> 5; j < kKoTJ; j += kThreads / kKwCols)  // (a row of vs per half wave: runs of <= 32 floats)
        vs[j * kKwCols + li] = (j < nj && c0 + li < c) ? vb[(size_t)(jt + j) * c + c0 + li] : 0.0f;
      __syncthreads();
      if (i0 >= M) continue;  // (wave uniform: a wave without rows stages and waits, and computes nothing)
      kw_f32x16 tacc[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tacc[t][r] = 0.0f;
      for (int j = 0; j < nj; j += 2) {  // (nj odd: the last step's upper half is j == nj <= 127, masked below)
        const int jj = j + h;
        const float* bp = xs + jj * DP;
        float r2[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float bk = bp[k];
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const float df = a[t][k] - bk;
            r2[t] = fmaf(df, df, r2[t]);
          }
        }
        const float bv = vs[jj * kKwCols + li];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float kv = jj < nj ? kf_g<FAMILY>(r2[t]) : 0.0f;
          tacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kv, bv, tacc[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t] += tacc[t];
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
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kr = 32 * t + 8 * (r >> 2) + (r & 3);
          if (ib + kr < M) {
            float res = os2 * acc[t][r];
            if (mode == LO_DIAG_FULL) res = fmaf(drow[kr], vrow[(size_t)kr * c], res);
            else if (mode == LO_DIAG_CONST) res = fmaf(dconst, vrow[(size_t)kr * c], res);
            out[(size_t)kr * c] = res;
          }
        }
      }
    }
  }
}

int kernel_mv_wide_run(const float* x1, const float* x2, const float* theta, int64_t tstride, int family, int64_t B,
                       int64_t M, int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y,
                       float* part, const int* stop, hipStream_t st) {
  const KoSweep w(B, M, N, D);
  float* p = w.s.js > 1 ? part : nullptr;
  if (M != N) dmode = LO_DIAG_NONE;
  LO_PROF_BEGIN("k_kernel_mv_wide", st);
  ko_dispatch(family, w.DP, [&](auto F, auto P) {
    hipLaunchKernelGGL((k_kernel_mv_wide<F(), P()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)tstride, (int)M,
                       (int)N, (int)D, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_kernel_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y,
                            stop, st);
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_mv_wide_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, c); });
}

int lo_kernel_mv_wide_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family)) return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kernel_mv_wide_run(x1, x2, theta, D + 1, family, B, M, N, D, v, c, d, diag_mode, y, part, nullptr,
                            (hipStream_t)stream);
}

}  // extern "C"
