// lo_kernel_mgrad.hip -- the matrix-free Matern-5/2 gradient kernel: the covariance of the values and the D partial
// derivatives of a Matern-5/2 GP at its points, D + 1 outputs per input (GPyTorch's Matern52KernelGrad).
// LO_OP_KERNEL_MGRAD_DIAG and the entry points lo_kernel_mgrad_mv_f32 / lo_kernel_mgrad_bilinear_f32 of lo_amd.h.  The
// n (D + 1) x n (D + 1) matrix is never in memory.
//
// Layout as in lo_kernel_grad.hip: row index i T + a, column index j T + b, T = D + 1, a, b = 0 the value, 1 .. D the
// derivative in coordinate a - 1 (of x1[i]) / b - 1 (of x2[j]).  With t_k = theta[k], u_k = t_k x1[i,k] - t_k x2[j,k]
// (scaled points differenced directly), q = r^2 = |u|^2, s = sqrt(5) r, E = exp(-s) and the three radial factors
//   g0 = (1 + s + s^2 / 3) E    g1 = -2 dg0/dq = (5 / 3) (1 + s) E    g2 = -2 dg1/dq = (25 / 3) E    (kf_mgrad_pair)
//   K[0,0] = os2 g0   K[0,b] = os2 t_b u_b g1   K[a,0] = -os2 t_a u_a g1   K[a,b] = os2 t_a t_b (g1 delta_ab - g2 u_a u_b)
// (the RBF gradient kernel is g0 = g1 = g2).  One v_sqrt_f32 and one v_exp_f32 per pair serve all (D + 1)^2 entries of the
// block and every column of the chunk; nothing is singular at r = 0.
// Product (k_kernel_mgrad_mv): one thread per data row i, tiles of x2 and of w (w[j,0] = v[j,0], w[j,b] = t_b v[j,b])
//   through LDS, u[DP] and g0, g1, g2 in registers.  Per pair and column sg = u . w[j,1:] (D FMAs), h = g1 w[j,0] + g2 sg,
//   y[i,0] += g0 w[j,0] + g1 sg,  y[i,a] += g1 w[j,a] - u_a h  (2 D + 4 FMAs); os2 and os2 t_a are applied once at the
//   store.  A thread holds (DP + 1) CC running sums and as many tile sums (a tile's sums are formed on their own, then added).
// Hyperparameters (k_kernel_mgrad_bilinear): S = sum_s U_s^T K V_s.  With Ut, Vt scaled as w above, per pair and column
//   al = u . Ut[i,1:], be = u . Vt[j,1:], G = Ut[i,1:] . Vt[j,1:], p00 = Ut[i,0] Vt[j,0], mid = Ut[i,0] be - al Vt[j,0] + G:
//     S / os2 = sum  g0 p00 + g1 mid - g2 al be
//   t_k d/dt_k acts on u_k (t_k du_k/dt_k = u_k), on Ut[i,k] and Vt[j,k] (each its own value) and on q (t_k dq/dt_k =
//   2 u_k^2, with dg0/dq = -g1 / 2, dg1/dq = -g2 / 2, dg2/dq = -g3 / 2, g3 = (25 sqrt(5) / 3) E / r):
//     t_k d al = 2 u_k Ut[i,k],  t_k d be = 2 u_k Vt[j,k],  t_k d G = 2 Ut[i,k] Vt[j,k],  t_k d g_m = -u_k^2 g_{m+1}
//     t_k dS/dt_k / os2 = sum  -u_k^2 P1 + 2 g1 (u_k Q1_k + G_k) - 2 g2 u_k Q2_k
//     P1 = g1 p00 + g2 mid - g3 al be,   Q1_k = Vt[j,k] Ut[i,0] - Ut[i,k] Vt[j,0],   G_k = Ut[i,k] Vt[j,k],
//     Q2_k = Ut[i,k] be + Vt[j,k] al     (each summed over the columns of the sweep)
//   g3 is the only factor with 1 / r; it multiplies al be u_k^2, of order r^4, and is taken as 0 for r^2 <= 1e-30, the
//   cut-off of covariance._dist (kf_mgrad_pair3).  The sweep runs twice over the columns of a pair -- first al, be and the
//   pair's two scalars, then per dimension Q1_k, G_k, Q2_k -- so that nothing of size DP lives across the pair but u and
//   the running sums.  One partial per workgroup by a fixed-order block sum, added in ascending order by k_kernel_bil_reduce.
// Few rows: the points j are split as in ko_shape; the partials of the product are added in ascending order by
// k_kernel_mv_reduce, which also applies + d o v.  No float atomics, no workgroup waits for another: equal bits per call.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_tile.h"

namespace lo {

// (the column chunks km_col_chunk / km_cols / km_bil_cols by the padded dimension: lo_kernel_shape.h)

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M T, c]
template <int DP, int CC>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_kernel_mgrad_mv(
    const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ theta, int M, int N, int D,
    const float* __restrict__ v, int c, const float* __restrict__ dd_ptr, int dd_mode, float* __restrict__ y,
    float* __restrict__ part, int jchunk, const int* __restrict__ stop) {
  if (stop && *stop) return;
  constexpr int TP = DP + 1;  // slots of a point: the value, then DP derivative slots (those beyond D hold 0)
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float ws[kKoTJ * CC * TP];  // [j][cc][slot]
  __shared__ float th[DP];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const int T = D + 1;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * T + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
  const float os2 = theta[b * T + D];
  const float* x2b = x2 + (size_t)b * N * D;
  const float* vb = v + (size_t)b * N * T * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += CC) {
    float acc[CC][TP];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc)
#pragma unroll
      for (int q = 0; q < TP; ++q) acc[cc][q] = 0.0f;
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
        const int j = e / DP, dd = e - j * DP;
        xs[e] = dd < D ? x2b[(size_t)(jt + j) * D + dd] * th[dd] : 0.0f;
      }
      // the tile of v, read in its memory order (j, slot, column) and scaled on the way in: slot b >= 1 times t_b
      for (int e = threadIdx.x; e < nj * TP * CC; e += kThreads) {
        const int j = e / (TP * CC), rem = e - j * (TP * CC);
        const int q = rem / CC, cc = rem - q * CC;
        float r = 0.0f;
        if (q < T && c0 + cc < c) {
          r = vb[((size_t)(jt + j) * T + q) * c + c0 + cc];
          if (q) r *= th[q - 1];
        }
        ws[(j * CC + cc) * TP + q] = r;
      }
      __syncthreads();
      float tacc[CC][TP];
#pragma unroll
      for (int cc = 0; cc < CC; ++cc)
#pragma unroll
        for (int q = 0; q < TP; ++q) tacc[cc][q] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float u[DP];
        float r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          u[k] = a[k] - xs[j * DP + k];
          r2 = fmaf(u[k], u[k], r2);
        }
        float g0, g1, g2;
        kf_mgrad_pair(r2, &g0, &g1, &g2);
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) {
          const float* w = ws + (j * CC + cc) * TP;
          float sg = 0.0f;
#pragma unroll
          for (int k = 0; k < DP; ++k) sg = fmaf(u[k], w[k + 1], sg);
          const float h = fmaf(g2, sg, g1 * w[0]);
          tacc[cc][0] = fmaf(g0, w[0], fmaf(g1, sg, tacc[cc][0]));
#pragma unroll
          for (int k = 0; k < DP; ++k) tacc[cc][k + 1] = fmaf(g1, w[k + 1], fmaf(-u[k], h, tacc[cc][k + 1]));
        }
      }
#pragma unroll
      for (int cc = 0; cc < CC; ++cc)
#pragma unroll
        for (int q = 0; q < TP; ++q) acc[cc][q] += tacc[cc][q];
    }
    if (live) {
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) {
        const int col = c0 + cc;
        if (col < c) {
#pragma unroll
          for (int q = 0; q < TP; ++q) {
            if (q < T) {
              const size_t row = ((size_t)b * M + i) * T + q;  // the full row i T + q of member b
              const size_t o = row * c + col;
              float r = (q ? os2 * th[q ? q - 1 : 0] : os2) * acc[cc][q];
              if (part) {
                part[(size_t)blockIdx.z * gridDim.y * M * T * c + o] = r;
              } else {
                if (dd_mode == LO_DIAG_FULL) r = fmaf(dd_ptr[row], v[o], r);
                else if (dd_mode == LO_DIAG_CONST) r = fmaf(dd_ptr[b], v[o], r);
                y[o] = r;
              }
            }
          }
        }
      }
    }
  }
}

// grid (row blocks, B, js); part [B, nblk = gridDim.x * gridDim.z, DP + 1]: slots k < DP the sums of t_k dS / dt_k / os2,
// slot DP the sum of S / os2 (the layout k_kernel_bil_reduce reads)
template <int DP, int TS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_kernel_mgrad_bilinear(
    const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ theta, int M, int N, int D,
    const float* __restrict__ U, const float* __restrict__ V, int t, float* __restrict__ part, int jchunk) {
  constexpr int TP = DP + 1;
  __shared__ __align__(16) float xs[kKoTJ * DP];
  __shared__ __align__(16) float vs[kKoTJ * TS * TP];  // [j][ss][slot]
  __shared__ float th[DP];
  __shared__ float red[4];
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  const int T = D + 1;
  if (threadIdx.x < DP) th[threadIdx.x] = (int)threadIdx.x < D ? theta[b * T + threadIdx.x] : 0.0f;
  __syncthreads();
  float a[DP], gacc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    a[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] * th[k] : 0.0f;
    gacc[k] = 0.0f;
  }
  KoKahan gos;  // the outputscale entry is ONE number per member, a sum of N M terms of both signs: compensated
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Ub = U + ((size_t)b * M + (live ? i : 0)) * T * t;
  const float* Vb = V + (size_t)b * N * T * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += TS) {
    float ut[TS][TP];  // the thread's rows of U, scaled as the tile of V is (a row beyond M: zeros, its pairs add nothing)
#pragma unroll
    for (int ss = 0; ss < TS; ++ss)
#pragma unroll
      for (int q = 0; q < TP; ++q) {
        float r = (live && q < T && s0 + ss < t) ? Ub[(size_t)q * t + s0 + ss] : 0.0f;
        if (q) r *= th[q ? q - 1 : 0];
        ut[ss][q] = r;
      }
    for (int jt = j0; jt < j1; jt += kKoTJ) {
      const int nj = min(kKoTJ, j1 - jt);
      __syncthreads();  // (the previous tile has been read)
      for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
        const int j = e / DP, dd = e - j * DP;
        xs[e] = dd < D ? x2b[(size_t)(jt + j) * D + dd] * th[dd] : 0.0f;
      }
      for (int e = threadIdx.x; e < nj * TP * TS; e += kThreads) {
        const int j = e / (TP * TS), rem = e - j * (TP * TS);
        const int q = rem / TS, ss = rem - q * TS;
        float r = 0.0f;
        if (q < T && s0 + ss < t) {
          r = Vb[((size_t)(jt + j) * T + q) * t + s0 + ss];
          if (q) r *= th[q - 1];
        }
        vs[(j * TS + ss) * TP + q] = r;
      }
      __syncthreads();
      float tacc[DP];  // (a tile's sums on their own, then added to the running ones, as in the product)
#pragma unroll
      for (int k = 0; k < DP; ++k) tacc[k] = 0.0f;
      for (int j = 0; j < nj; ++j) {
        float u[DP];
        float r2 = 0.0f;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          u[k] = a[k] - xs[j * DP + k];
          r2 = fmaf(u[k], u[k], r2);
        }
        float g0, g1, g2, g3;
        kf_mgrad_pair3(r2, &g0, &g1, &g2, &g3);
        // first pass over the columns: al, be per column; the pair's S / os2 (F) and the factor P1 of -u_k^2
        float al[TS], be[TS];
        float F = 0.0f, P1 = 0.0f;
#pragma unroll
        for (int ss = 0; ss < TS; ++ss) {
          const float* w = vs + (j * TS + ss) * TP;
          float sa = 0.0f, sb = 0.0f, G = 0.0f;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            sa = fmaf(u[k], ut[ss][k + 1], sa);
            sb = fmaf(u[k], w[k + 1], sb);
            G = fmaf(ut[ss][k + 1], w[k + 1], G);
          }
          al[ss] = sa;
          be[ss] = sb;
          const float p00 = ut[ss][0] * w[0];
          const float mid = fmaf(ut[ss][0], sb, fmaf(-sa, w[0], G));
          const float ab = sa * sb;
          F += fmaf(g0, p00, fmaf(g1, mid, -g2 * ab));
          P1 += fmaf(g1, p00, fmaf(g2, mid, -g3 * ab));
        }
        gos.add(1.0f, F);
        // second pass, per dimension: Q1_k, G_k, Q2_k summed over the columns, then the pair's term of t_k dS / dt_k
        const float g1x2 = 2.0f * g1, g2x2 = 2.0f * g2;
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          float q1 = 0.0f, gk = 0.0f, q2 = 0.0f;
#pragma unroll
          for (int ss = 0; ss < TS; ++ss) {
            const float* w = vs + (j * TS + ss) * TP;
            const float wv = w[k + 1], uv = ut[ss][k + 1];
            q1 = fmaf(wv, ut[ss][0], q1);
            q1 = fmaf(-uv, w[0], q1);
            gk = fmaf(uv, wv, gk);
            q2 = fmaf(uv, be[ss], q2);
            q2 = fmaf(wv, al[ss], q2);
          }
          const float lin = fmaf(g1x2, q1, -g2x2 * q2);
          tacc[k] += fmaf(u[k], fmaf(-u[k], P1, lin), g1x2 * gk);
        }
      }
#pragma unroll
      for (int k = 0; k < DP; ++k) gacc[k] += tacc[k];
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
  float* out = part + ((size_t)b * nblk + blk) * (DP + 1);
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    const float sum = block_sum256(gacc[k], red);
    if (threadIdx.x == 0) out[k] = sum;
  }
  const float sum = block_sum256(gos.s, red);
  if (threadIdx.x == 0) out[DP] = sum;
}

// arguments both entry points and the descriptor are held to (all sizes already positive); cols = c or t
static bool km_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t cols) {
  return D <= LO_KERNEL_GRAD_MAX_DIM && B <= 65535 && M * (D + 1) <= 0x7ffffe00 && N * (D + 1) <= 0x7ffffe00 &&
         cols <= 0x7fffffff / (D + 1);
}

// the product on validated arguments; part: the partials [js, B, M, (D + 1) c] of a split member
static int km_mv_run(const float* x1, const float* x2, const float* theta, int64_t B, int64_t M, int64_t N, int64_t D,
                     const float* v, int64_t c, const float* d, int dmode, float* y, float* part, const int* stop,
                     hipStream_t st) {
  const KoSweep w(B, M, N, D);
  const int CC = km_col_chunk(w.DP, c);
  const int64_t T = D + 1;
  float* p = w.s.js > 1 ? part : nullptr;
  LO_PROF_BEGIN("k_kernel_mgrad_mv", st);
  ko_pick(kg_dims{}, w.DP, [&](auto P) {  // (the column list depends on the padded dimension)
    ko_pick(km_cols<P()>{}, CC, [&](auto C) {
      hipLaunchKernelGGL((k_kernel_mgrad_mv<P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M, (int)N, (int)D,
                         v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)  // (rows of c elements: the full diagonal of the reduction is indexed by o / c = the full row i T + a)
    return ko_reduce_splits("k_kernel_mgrad_mv_reduce", p, w.s.js, (size_t)M * T * c, (size_t)B * M * T * c, (int)c, d,
                            dmode, v, y, stop, st);
  return LO_OK;
}

int kernel_mgrad_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1) return LO_ERR_BADARG;
  if (op->N < 1 || op->N % (op->R + 1) != 0) return LO_ERR_BADARG;
  if (op->R > LO_KERNEL_GRAD_MAX_DIM) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

int kernel_mgrad_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_mgrad_desc_check(&op)) return rc;
  const int64_t n = op.N / (op.R + 1);
  if (!km_shape_ok(op.B, n, n, op.R, pl->c)) return LO_ERR_UNSUPPORTED;
  pl->kg.part = ko_split_layout<float>(*ar, op.B, n, n, (op.R + 1) * pl->c);
  return LO_OK;
}

int kernel_mgrad_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const int64_t n = op.N / (op.R + 1);
  return km_mv_run(op.A0, op.A0, op.A1, op.B, n, n, op.R, v, pl->c, op.d, op.diag_mode, y, pl->kg.part, stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_mgrad_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !km_shape_ok(B, M, N, D, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, (D + 1) * c); });
}

int lo_kernel_mgrad_mv_f32(const float* x1, const float* x2, const float* theta, int64_t B, int64_t M, int64_t N, int64_t D,
                           const float* v, int64_t c, const float* d, int32_t diag_mode, float* y, void* ws,
                           size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c)) return LO_ERR_BADARG;
  // (a diagonal term only on a square operator, and then with its operand)
  if (!ko_diag_ok(diag_mode, d, true) || (diag_mode != LO_DIAG_NONE && M != N)) return LO_ERR_BADARG;
  if (!km_shape_ok(B, M, N, D, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, (D + 1) * c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return km_mv_run(x1, x2, theta, B, M, N, D, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

size_t lo_kernel_mgrad_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !km_shape_ok(B, M, N, D, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_mgrad_bilinear_f32(const float* x1, const float* x2, const float* theta, int64_t B, int64_t M, int64_t N,
                                 int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t)) return LO_ERR_BADARG;
  if (!km_shape_ok(B, M, N, D, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_bil_layout<float>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kernel_mgrad_bilinear", st);
  ko_pick(kg_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_kernel_mgrad_bilinear<P(), km_bil_cols(P())>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M,
                       (int)N, (int)D, U, V, (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return ko_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, theta, g_theta, st);
}

}  // extern "C"
