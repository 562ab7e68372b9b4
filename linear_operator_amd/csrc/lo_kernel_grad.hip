// lo_kernel_grad.hip -- the matrix-free RBF gradient kernel: the covariance of the values and the D partial derivatives
// of a GP at its points, D + 1 outputs per input (the case kernel_linear_operator.py:130-133 of the reference names for
// num_outputs_per_input; GPyTorch's RBFKernelGrad).  LO_OP_KERNEL_GRAD_DIAG and the entry points lo_kernel_grad_mv_f32 /
// lo_kernel_grad_bilinear_f32 of lo_amd.h.  The n (D + 1) x n (D + 1) matrix is never in memory.
//
// Row index i T + a and column index j T + b with T = D + 1, the data index slowest: a, b = 0 the value, 1 .. D the
// derivative in coordinate a - 1 (of x1[i]) / b - 1 (of x2[j]).  With t_k = theta[k], u_k = t_k x1[i,k] - t_k x2[j,k]
// (scaled points differenced directly), e = exp(-|u|^2 / 2):
//   K[0,0] = os2 e   K[0,b] = os2 t_b u_b e   K[a,0] = -os2 t_a u_a e   K[a,b] = os2 t_a t_b (delta_ab - u_a u_b) e
// Product (k_kernel_grad_mv): the sweep of k_kernel_kron_mv (lo_kernel_kron.hip) with the "task factor" a rank-one-plus-
//   diagonal function of the pair.  The tile of v is staged as w[j,0] = v[j,0], w[j,b] = t_b v[j,b]; per pair and column
//   s = w[j,0] + sum_b u_b w[j,b] (D FMAs), then y[i,0] += e s and y[i,a] += e (w[j,a] - u_a s) (2 D + 1 FMAs); the scales
//   os2 and os2 t_a are applied once at the store.  Nothing of size D^2 is formed.  A thread holds (DP + 1) CC running
//   sums and as many tile sums (a tile's sums are formed on their own, then added).
// Hyperparameters (k_kernel_grad_bilinear): S = sum_s U_s^T K V_s.  With Ut, Vt scaled as w above, per pair and column
//   alpha = u . Ut[i,1:], beta = u . Vt[j,1:], A = Ut[i,0] - alpha, Bv = Vt[j,0] + beta, P = A Bv + Ut[i,1:] . Vt[j,1:]:
//   S = os2 sum e P,  t_k dS/dt_k = os2 sum e [-u_k^2 P + 2 u_k (Vt[j,k] A - Ut[i,k] Bv) + 2 Ut[i,k] Vt[j,k]]
//   one partial per workgroup by a fixed-order block sum, added in ascending order by k_kernel_bil_reduce.
// Few rows: the points j are split as in ko_shape; the partials of the product are added in ascending order by
// k_kernel_mv_reduce, which also applies + d o v.  No float atomics, no workgroup waits for another: equal bits per call.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"

namespace lo {

// (the column chunks kg_col_chunk / kg_cols / kg_bil_cols by the padded dimension: lo_kernel_shape.h)

// grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else partial products [js, B, M T, c]
template <int FAMILY, int DP, int CC>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_kernel_grad_mv(
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
        const float e = kf_grad_pair<FAMILY>(r2);
#pragma unroll
        for (int cc = 0; cc < CC; ++cc) {
          const float* w = ws + (j * CC + cc) * TP;
          float s = w[0];
#pragma unroll
          for (int k = 0; k < DP; ++k) s = fmaf(u[k], w[k + 1], s);
          tacc[cc][0] = fmaf(e, s, tacc[cc][0]);
#pragma unroll
          for (int k = 0; k < DP; ++k) tacc[cc][k + 1] = fmaf(e, fmaf(-u[k], s, w[k + 1]), tacc[cc][k + 1]);
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
template <int FAMILY, int DP, int TS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3))) void k_kernel_grad_bilinear(
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
  float gos = 0.0f, gos_c = 0.0f;
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Ub = U + ((size_t)b * M + (live ? i : 0)) * T * t;
  const float* Vb = V + (size_t)b * N * T * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += TS) {
    float ut[TS][TP];  // the thread's rows of U, scaled as the tile of V is
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
        const float e = kf_grad_pair<FAMILY>(r2);
        float A[TS], Bv[TS];
        float P = 0.0f;  // sum over the columns of A Bv + Ut[1:] . Vt[1:]
#pragma unroll
        for (int ss = 0; ss < TS; ++ss) {
          const float* w = vs + (j * TS + ss) * TP;
          float al = 0.0f, be = 0.0f;
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            al = fmaf(u[k], ut[ss][k + 1], al);
            be = fmaf(u[k], w[k + 1], be);
          }
          A[ss] = ut[ss][0] - al;
          Bv[ss] = w[0] + be;
          P = fmaf(A[ss], Bv[ss], P);
        }
        float q2[DP], g2[DP];  // per dimension: sum_s (Vt[j,k] A - Ut[i,k] Bv) and sum_s Ut[i,k] Vt[j,k]
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          float qk = 0.0f, gk = 0.0f;
#pragma unroll
          for (int ss = 0; ss < TS; ++ss) {
            const float wv = vs[(j * TS + ss) * TP + k + 1];
            qk = fmaf(wv, A[ss], qk);
            qk = fmaf(-ut[ss][k + 1], Bv[ss], qk);
            gk = fmaf(ut[ss][k + 1], wv, gk);
          }
          q2[k] = qk;
          g2[k] = gk;
          P += gk;
        }
        {  // the outputscale entry is ONE number per member, a sum of N M terms of both signs: compensated (Kahan)
          const float term = fmaf(e, P, -gos_c);
          const float next = gos + term;
          gos_c = (next - gos) - term;
          gos = next;
        }
#pragma unroll
        for (int k = 0; k < DP; ++k) {
          const float inner = fmaf(u[k], fmaf(-u[k], P, 2.0f * q2[k]), 2.0f * g2[k]);
          tacc[k] = fmaf(e, inner, tacc[k]);
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
  const float sum = block_sum256(gos, red);
  if (threadIdx.x == 0) out[DP] = sum;
}

// arguments both entry points and the descriptor are held to (all sizes already positive); cols = c or t
static bool kg_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t cols) {
  return D <= LO_KERNEL_GRAD_MAX_DIM && B <= 65535 && M * (D + 1) <= 0x7ffffe00 && N * (D + 1) <= 0x7ffffe00 &&
         cols <= 0x7fffffff / (D + 1);
}

// the product on validated arguments (family RBF); part: the partials [js, B, M, (D + 1) c] of a split member
static int kg_mv_run(const float* x1, const float* x2, const float* theta, int64_t B, int64_t M, int64_t N, int64_t D,
                     const float* v, int64_t c, const float* d, int dmode, float* y, float* part, const int* stop,
                     hipStream_t st) {
  const KoSweep w(B, M, N, D);
  const int CC = kg_col_chunk(w.DP, c);
  const int64_t T = D + 1;
  float* p = w.s.js > 1 ? part : nullptr;
  LO_PROF_BEGIN("k_kernel_grad_mv", st);
  ko_pick(kg_dims{}, w.DP, [&](auto P) {  // (the column list depends on the padded dimension)
    ko_pick(kg_cols<P()>{}, CC, [&](auto C) {
      hipLaunchKernelGGL((k_kernel_grad_mv<LO_KERNEL_RBF, P(), C()>), w.grid, dim3(kThreads), 0, st, x1, x2, theta, (int)M,
                         (int)N, (int)D, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
    });
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)  // (rows of c elements: the full diagonal of the reduction is indexed by o / c = the full row i T + a)
    return ko_reduce_splits("k_kernel_grad_mv_reduce", p, w.s.js, (size_t)M * T * c, (size_t)B * M * T * c, (int)c, d,
                            dmode, v, y, stop, st);
  return LO_OK;
}

int kernel_grad_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1 || !ko_family_ok(op->n2)) return LO_ERR_BADARG;
  if (op->N < 1 || op->N % (op->R + 1) != 0) return LO_ERR_BADARG;
  if (op->R > LO_KERNEL_GRAD_MAX_DIM || op->n2 != LO_KERNEL_RBF) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

int kernel_grad_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = kernel_grad_desc_check(&op)) return rc;
  const int64_t n = op.N / (op.R + 1);
  if (!kg_shape_ok(op.B, n, n, op.R, pl->c)) return LO_ERR_UNSUPPORTED;
  pl->kg.part = ko_split_layout<float>(*ar, op.B, n, n, (op.R + 1) * pl->c);
  return LO_OK;
}

int kernel_grad_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const int64_t n = op.N / (op.R + 1);
  return kg_mv_run(op.A0, op.A0, op.A1, op.B, n, n, op.R, v, pl->c, op.d, op.diag_mode, y, pl->kg.part, stop, st);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_grad_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !kg_shape_ok(B, M, N, D, c)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, (D + 1) * c); });
}

int lo_kernel_grad_mv_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const float* v, int64_t c, const float* d, int32_t diag_mode, float* y,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !v || !y || !ko_args_ok(B, M, N, D, c) || !ko_family_ok(family)) return LO_ERR_BADARG;
  // (a diagonal term only on a square operator, and then with its operand)
  if (!ko_diag_ok(diag_mode, d, true) || (diag_mode != LO_DIAG_NONE && M != N)) return LO_ERR_BADARG;
  if (family != LO_KERNEL_RBF || !kg_shape_ok(B, M, N, D, c)) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, (D + 1) * c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return kg_mv_run(x1, x2, theta, B, M, N, D, v, c, d, diag_mode, y, part, nullptr, (hipStream_t)stream);
}

size_t lo_kernel_grad_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !kg_shape_ok(B, M, N, D, t)) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_bil_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_grad_bilinear_f32(const float* x1, const float* x2, const float* theta, int32_t family, int64_t B, int64_t M,
                                int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ko_family_ok(family))
    return LO_ERR_BADARG;
  if (family != LO_KERNEL_RBF || !kg_shape_ok(B, M, N, D, t)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_bil_layout<float>(ar, B, M, N, D);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  LO_PROF_BEGIN("k_kernel_grad_bilinear", st);
  ko_pick(kg_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_kernel_grad_bilinear<LO_KERNEL_RBF, P(), kg_bil_cols(P())>), w.grid, dim3(kThreads), 0, st, x1, x2,
                       theta, (int)M, (int)N, (int)D, U, V, (int)t, part, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return ko_bil_reduce(part, w.s.rb * w.s.js, w.DP, B, D, theta, g_theta, st);
}

}  // extern "C"

