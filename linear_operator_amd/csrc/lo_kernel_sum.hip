// lo_kernel_sum.hip -- sums of matrix-free kernel operators over the SAME points in one pass,
//   K_ij = sum_t theta[t][D] g_{f_t}(r_t,ij),   r_t,ij^2 = sum_d (theta[t][d] (x1[i, d] - x2[j, d]))^2,   1 <= T <= 4 terms,
// the kind LO_OP_KERNEL_SUM_DIAG and the entry points lo_kernel_sum_mv_f32 / lo_kernel_sum_bilinear_f32 /
// lo_kernel_sum_points_grad_f32 of lo_amd.h.  The structure is that of lo_kernel_op.hip (a thread owns a row, tiles of x2
// and of v stream through LDS, column splits for few rows, fixed-order sums, no float atomics, r^2 from direct
// differences); the launch shape, the padded sizes and the reduction of the splits are shared (lo_kernel_shape.h).
//
// What is new.  The tile of x2 is staged once PER TERM, scaled by that term's inverse lengthscales (T DP floats per
// point); the tile of v (or of V) is staged once.  A tile is walked in sub-tiles of 8 pairs: the term loop runs OUTSIDE
// the sub-tile, so a term's family is switched on once per 8 pairs and the loop over the pairs inside is a template of
// the family; the thread scales its own point for the term (DP multiplications per 8 pairs) and the 8 kernel values
// sum_t os2_t g_t(r_t) collect in registers.  Only then do the CC column FMAs run, once per pair for all terms.
//   Product: kv[8] -> the tile's sums -> the running sums, as in k_kernel_mv.
//   Derivative: W_ij = sum_s U[i, s] V[j, s] for the 8 pairs once (kept in LDS slots of the thread), then per term the
//     sub-tile's sums of W h_t (a_d - b_d)^2 and the compensated sum of W g_t, added to the term's running sums.  A
//     thread holds TT (DP + 1) running sums: TT = 4 terms per sweep for D <= 16, 2 for 16 < D <= 32 (3 or 4 terms of
//     that width take two sweeps).
//   Points: per term the sub-tile's sums of W h_t (a_d - b_d), added with the factor os2_t theta_t[d] to ONE running sum
//     per dimension -- the gradient of the sum of the terms.
// Rows of a ragged last sub-tile are staged as zeros (points, v and V): they add exactly 0.
// The product is fused where that was measured faster -- more than 4 columns; a narrower one runs the single-term kernel
// of lo_kernel_op.hip once per term, inside ksum_mv_run (ks_mv_fused; DESIGN.md section 6m has the table).
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_shape.h"
#include "lo_kernel_terms.h"

namespace lo {

constexpr int kKsCC = 16;  // columns per sweep of the fused product (narrower right-hand sides: the per-term route)

// terms per sweep of the derivative (a thread's running sums: TT (DP + 1))
template <int DP>
constexpr int ks_bil_terms() { return DP == 32 ? 2 : 4; }

static size_t ks_lds_bytes(int T, int DP, int cols) {
  const int TJ = DP == 32 ? kKoTJ / 2 : kKoTJ;
  return ((size_t)T * TJ * DP + (size_t)TJ * cols + (size_t)T * (DP + 1)) * sizeof(float);
}

// the tile of v (or V): vs[TJ][COLS] of the columns [c0, c0 + COLS), zeros beyond c and in the rows [nj, njp)
template <int COLS>
__device__ __forceinline__ void ks_stage_cols(const float* __restrict__ vb, int c, int c0, int jt, int nj, int njp,
                                              float* __restrict__ vs) {
  for (int e = threadIdx.x; e < njp * COLS; e += kThreads) {
    const int j = e / COLS, cc = e - j * COLS;
    vs[e] = (j < nj && c0 + cc < c) ? vb[(size_t)(jt + j) * c + c0 + cc] : 0.0f;
  }
}

// ---- the loops over the 8 pairs of a sub-tile, one instantiation per family (the product's: ks_sub_g, lo_kernel_terms.h)
// sacc[k] += W h (a_k - b_k)^2, the compensated (Kahan) sum gos += W g
template <int FAMILY, int DP>
__device__ __forceinline__ void ks_sub_bil(const float (&at)[DP], const float* __restrict__ xt,
                                           const float* __restrict__ wl, float (&sacc)[DP], float& gos,
                                           float& gos_c) {
#pragma unroll 2
  for (int jj = 0; jj < kKsJS; ++jj) {
    const float wj = wl[jj * kThreads];
    float sd[DP];
    float r2 = 0.0f;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      sd[k] = at[k] - xt[jj * DP + k];
      r2 = fmaf(sd[k], sd[k], r2);
    }
    float g, h;
    kf_gh<FAMILY>(r2, &g, &h);
    const float term = fmaf(wj, g, -gos_c);
    const float next = gos + term;
    gos_c = (next - gos) - term;
    gos = next;
    const float wh = wj * h;
#pragma unroll
    for (int k = 0; k < DP; ++k) sacc[k] = fmaf(wh * sd[k], sd[k], sacc[k]);
  }
}

// sacc[k] += W h (a_k - b_k)
template <int FAMILY, int DP>
__device__ __forceinline__ void ks_sub_pg(const float (&at)[DP], const float* __restrict__ xt,
                                          const float* __restrict__ wl, float (&sacc)[DP]) {
#pragma unroll 2
  for (int jj = 0; jj < kKsJS; ++jj) {
    const float wj = wl[jj * kThreads];
    float sd[DP];
    float r2 = 0.0f;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
      sd[k] = at[k] - xt[jj * DP + k];
      r2 = fmaf(sd[k], sd[k], r2);
    }
    float g, h;
    kf_gh<FAMILY>(r2, &g, &h);
    const float wh = wj * h;
#pragma unroll
    for (int k = 0; k < DP; ++k) sacc[k] = fmaf(wh, sd[k], sacc[k]);
  }
}

// W of the 8 pairs of a sub-tile from the thread's row of U and the staged rows of V, formed once for all terms.  The
// thread keeps them in LDS slots of its own, wl[jj * 256] (8 registers indexed by the pair would force the loop over the
// pairs to be unrolled whole, and with it 8 sets of differences to be live at once); no barrier: nobody else reads them.
__device__ __forceinline__ void ks_sub_w(const float (&u)[kKoTS], const float* __restrict__ vt, float* __restrict__ wl) {
#pragma unroll
  for (int jj = 0; jj < kKsJS; ++jj) {
    float s = 0.0f;
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) s = fmaf(u[ss], vt[jj * kKoTS + ss], s);
    wl[jj * kThreads] = s;
  }
}

// ---- the product: grid (row blocks, B, js); part == nullptr: y is written with the diagonal term, else the partial
// products [js, B, M, c].  `fams`: the family codes, four bits per term, term 0 lowest.  Dynamic LDS:
// ks_lds_bytes(T, DP, CC)
template <int DP, int CC>
__global__ __launch_bounds__(kThreads) void k_ksum_mv(const float* __restrict__ x1, const float* __restrict__ x2,
                                                      const float* __restrict__ theta, unsigned fams, int T, int M, int N,
                                                      int D, const float* __restrict__ v, int c,
                                                      const float* __restrict__ dd_ptr, int dd_mode,
                                                      float* __restrict__ y, float* __restrict__ part, int jchunk,
                                                      const int* __restrict__ stop) {
  if (stop && *stop) return;
  extern __shared__ __align__(16) float ks_smem[];
  constexpr int TJ = ks_tile<DP>();
  float* xs = ks_smem;                  // [T][TJ][DP]
  float* vs = xs + (size_t)T * TJ * DP; // [TJ][CC]
  float* th = vs + TJ * CC;             // [T][DP + 1]
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  ks_stage_theta<DP>(theta + (size_t)b * T * (D + 1), D, 0, T, th);
  __syncthreads();
  float araw[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) araw[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
  const float* x2b = x2 + (size_t)b * N * D;
  const float* vb = v + (size_t)b * N * c;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int c0 = 0; c0 < c; c0 += CC) {
    float acc[CC];
#pragma unroll
    for (int cc = 0; cc < CC; ++cc) acc[cc] = 0.0f;
    for (int jt = j0; jt < j1; jt += TJ) {
      const int nj = min(TJ, j1 - jt);
      const int njp = (nj + kKsJS - 1) / kKsJS * kKsJS;
      __syncthreads();  // (the previous tile has been read)
      ks_stage_points<DP>(x2b, th, D, T, jt, nj, njp, xs);
      ks_stage_cols<CC>(vb, c, c0, jt, nj, njp, vs);
      __syncthreads();
      float tacc[CC];
#pragma unroll
      for (int cc = 0; cc < CC; ++cc) tacc[cc] = 0.0f;
      for (int js = 0; js < njp; js += kKsJS) {
        float kv[kKsJS];
#pragma unroll
        for (int jj = 0; jj < kKsJS; ++jj) kv[jj] = 0.0f;
        for (int t = 0; t < T; ++t) {
          float at[DP];
#pragma unroll
          for (int k = 0; k < DP; ++k) at[k] = ks_scale(araw[k], th[t * (DP + 1) + k]);
          const float os2 = th[t * (DP + 1) + DP];
          const float* xt = xs + ((size_t)t * TJ + js) * DP;
#define KS_CALL(F_) ks_sub_g<F_, DP>(at, xt, os2, kv)
          KS_FAMILY_SWITCH((fams >> (4 * t)) & 15u, KS_CALL)
#undef KS_CALL
        }
#pragma unroll
        for (int jj = 0; jj < kKsJS; ++jj) {
#pragma unroll
          for (int cc = 0; cc < CC; ++cc) tacc[cc] = fmaf(kv[jj], vs[(js + jj) * CC + cc], tacc[cc]);
        }
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
          float r = acc[cc];
          if (part) {
            part[(size_t)blockIdx.z * gridDim.y * M * c + o] = r;
          } else {
            if (dd_mode == LO_DIAG_FULL) r = fmaf(dd_ptr[(size_t)b * M + i], v[o], r);
            else if (dd_mode == LO_DIAG_CONST) r = fmaf(dd_ptr[b], v[o], r);
            y[o] = r;
          }
        }
      }
    }
  }
}

// ---- the derivative of the terms [t0, t0 + nt), nt <= TT: grid (row blocks, B, js); part [B, nblk, T, DP + 1] with
// nblk = gridDim.x * gridDim.z.  Dynamic LDS: ks_lds_bytes(nt, DP, kKoTS)
template <int DP>
__global__ __launch_bounds__(kThreads) void k_ksum_bil(const float* __restrict__ x1, const float* __restrict__ x2,
                                                       const float* __restrict__ theta, unsigned fams, int T, int t0,
                                                       int nt, int M, int N, int D, const float* __restrict__ U,
                                                       const float* __restrict__ V, int t, float* __restrict__ part,
                                                       int jchunk) {
  extern __shared__ __align__(16) float ks_smem[];
  __shared__ float red[4];
  __shared__ float wsl[kKsJS * kThreads];
  float* wl = wsl + threadIdx.x;
  constexpr int TJ = ks_tile<DP>();
  constexpr int TT = ks_bil_terms<DP>();
  float* xs = ks_smem;                   // [nt][TJ][DP]
  float* vs = xs + (size_t)nt * TJ * DP; // [TJ][kKoTS]
  float* th = vs + TJ * kKoTS;           // [nt][DP + 1]
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  ks_stage_theta<DP>(theta + (size_t)b * T * (D + 1), D, t0, nt, th);
  __syncthreads();
  float araw[DP], gacc[TT][DP], gos[TT], gos_c[TT];
#pragma unroll
  for (int k = 0; k < DP; ++k) araw[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    gos[tt] = gos_c[tt] = 0.0f;
#pragma unroll
    for (int k = 0; k < DP; ++k) gacc[tt][k] = 0.0f;
  }
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += TJ) {
      const int nj = min(TJ, j1 - jt);
      const int njp = (nj + kKsJS - 1) / kKsJS * kKsJS;
      __syncthreads();
      ks_stage_points<DP>(x2b, th, D, nt, jt, nj, njp, xs);
      ks_stage_cols<kKoTS>(Vb, t, s0, jt, nj, njp, vs);
      __syncthreads();
      for (int js = 0; js < njp; js += kKsJS) {
        ks_sub_w(u, vs + js * kKoTS, wl);
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
          if (tt < nt) {
            float at[DP], sacc[DP];
#pragma unroll
            for (int k = 0; k < DP; ++k) {
              at[k] = ks_scale(araw[k], th[tt * (DP + 1) + k]);
              sacc[k] = 0.0f;
            }
            const float* xt = xs + ((size_t)tt * TJ + js) * DP;
#define KS_CALL(F_) ks_sub_bil<F_, DP>(at, xt, wl, sacc, gos[tt], gos_c[tt])
            KS_FAMILY_SWITCH((fams >> (4 * (t0 + tt))) & 15u, KS_CALL)
#undef KS_CALL
#pragma unroll
            for (int k = 0; k < DP; ++k) gacc[tt][k] += sacc[k];  // (a sub-tile's sums on their own, then the running ones)
          }
        }
      }
    }
  }
  const size_t blk = (size_t)blockIdx.z * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.z;
#pragma unroll
  for (int tt = 0; tt < TT; ++tt) {
    if (tt < nt) {  // (uniform: every thread takes part in the block sums)
      float* out = part + (((size_t)b * nblk + blk) * T + t0 + tt) * (DP + 1);
#pragma unroll
      for (int k = 0; k < DP; ++k) {
        const float sum = block_sum256(gacc[tt][k], red);
        if (threadIdx.x == 0) out[k] = sum;
      }
      const float sum = block_sum256(gos[tt], red);
      if (threadIdx.x == 0) out[DP] = sum;
    }
  }
}

// g_theta[b, t, q] from the nblk partials in ascending order: q < D: os2_t / theta_t[q] times the sum, q == D: the sum
__global__ __launch_bounds__(kThreads) void k_ksum_bil_reduce(const float* __restrict__ part, int nblk, int DP, int D,
                                                              int T, const float* __restrict__ theta,
                                                              float* __restrict__ g_theta) {
  const int64_t b = blockIdx.x;
  const int e = threadIdx.x;
  if (e >= T * (D + 1)) return;
  const int tm = e / (D + 1), q = e - tm * (D + 1);
  const int slot = q < D ? q : DP;
  const float* p = part + ((size_t)b * nblk * T + tm) * (DP + 1) + slot;
  float s = 0.0f;
  for (int k = 0; k < nblk; ++k) s += p[(size_t)k * T * (DP + 1)];
  const float* th = theta + ((size_t)b * T + tm) * (D + 1);
  if (q < D) s = th[q] != 0.0f ? s * th[D] / th[q] : 0.0f;
  g_theta[((size_t)b * T + tm) * (D + 1) + q] = s;
}

// ---- the gradient of the points x1, summed over the terms: grid (row blocks, B, js); `out` is g_x1 [B, M, D] when
// gridDim.z == 1, else the partials [js, B, M, D] of the column splits.  Dynamic LDS: ks_lds_bytes(T, DP, kKoTS)
template <int DP>
__global__ __launch_bounds__(kThreads) void k_ksum_pgrad(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ theta, unsigned fams, int T, int M,
                                                         int N, int D, const float* __restrict__ U,
                                                         const float* __restrict__ V, int t, float* __restrict__ out,
                                                         int jchunk) {
  extern __shared__ __align__(16) float ks_smem[];
  __shared__ float wsl[kKsJS * kThreads];
  float* wl = wsl + threadIdx.x;
  constexpr int TJ = ks_tile<DP>();
  float* xs = ks_smem;                  // [T][TJ][DP]
  float* vs = xs + (size_t)T * TJ * DP; // [TJ][kKoTS]
  float* th = vs + TJ * kKoTS;          // [T][DP + 1]
  const int64_t b = blockIdx.y;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < M;
  ks_stage_theta<DP>(theta + (size_t)b * T * (D + 1), D, 0, T, th);
  __syncthreads();
  float araw[DP], acc[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    araw[k] = (live && k < D) ? x1[((size_t)b * M + i) * D + k] : 0.0f;
    acc[k] = 0.0f;
  }
  const float* x2b = x2 + (size_t)b * N * D;
  const float* Vb = V + (size_t)b * N * t;
  const int j0 = blockIdx.z * jchunk, j1 = min(N, j0 + jchunk);
  for (int s0 = 0; s0 < t; s0 += kKoTS) {
    float u[kKoTS];
#pragma unroll
    for (int ss = 0; ss < kKoTS; ++ss) u[ss] = (live && s0 + ss < t) ? U[((size_t)b * M + i) * t + s0 + ss] : 0.0f;
    for (int jt = j0; jt < j1; jt += TJ) {
      const int nj = min(TJ, j1 - jt);
      const int njp = (nj + kKsJS - 1) / kKsJS * kKsJS;
      __syncthreads();
      ks_stage_points<DP>(x2b, th, D, T, jt, nj, njp, xs);
      ks_stage_cols<kKoTS>(Vb, t, s0, jt, nj, njp, vs);
      __syncthreads();
      for (int js = 0; js < njp; js += kKsJS) {
        ks_sub_w(u, vs + js * kKoTS, wl);
        for (int tm = 0; tm < T; ++tm) {
          float at[DP], sacc[DP];
#pragma unroll
          for (int k = 0; k < DP; ++k) {
            at[k] = ks_scale(araw[k], th[tm * (DP + 1) + k]);
            sacc[k] = 0.0f;
          }
          const float os2 = th[tm * (DP + 1) + DP];
          const float* xt = xs + ((size_t)tm * TJ + js) * DP;
#define KS_CALL(F_) ks_sub_pg<F_, DP>(at, xt, wl, sacc)
          KS_FAMILY_SWITCH((fams >> (4 * tm)) & 15u, KS_CALL)
#undef KS_CALL
#pragma unroll
          for (int k = 0; k < DP; ++k) acc[k] = fmaf(os2 * th[tm * (DP + 1) + k], sacc[k], acc[k]);
        }
      }
    }
  }
  if (live) {
    float* o = out + ((size_t)blockIdx.z * gridDim.y * M + (size_t)b * M + i) * D;
#pragma unroll
    for (int k = 0; k < DP; ++k)
      if (k < D) o[k] = acc[k];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static bool ks_terms_ok(int64_t T) { return T >= 1 && T <= LO_KERNEL_MAX_TERMS; }

// the packed family codes (four bits per term, term 0 lowest) of a host array, or -1 for an unknown family
static int64_t ks_pack(const int32_t* families, int64_t T) {
  int64_t packed = 0;
  for (int64_t t = 0; t < T; ++t) {
    if (!ko_family_ok(families[t])) return -1;
    packed |= (int64_t)families[t] << (4 * t);
  }
  return packed;
}

// The route of the product.  Measured on the MI355X (tools/mb_kernel_sum.py): with 16 columns per
// sweep the fused kernel takes 0.77 - 0.85 of the per-term route, with ONE column 1.06 - 1.24 of it -- the distances and
// exponentials are the same work either way, the fusion saves only the (T - 1) CC column FMAs and stagings of v and pays
// for the term loop.  So c <= 4 (the 1- and 4-column sweeps of lo_kernel_op.hip; 4 not measured, placed by the same
// count) and a single term run the single-term kernel once per term, the terms added in order; anything wider is fused.
static bool ks_mv_fused(int64_t T, int64_t c) { return T > 1 && ko_col_chunk(c) == kKsCC; }

struct KsMvBufs {
  float* part;  // [js, B, M, c] partial products of a split member, else nullptr
  float* ytmp;  // per-term route, T > 1: [B, M, c], a term beyond the first before it is added onto y
};

// the one layout of the product's workspace
static KsMvBufs ks_mv_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t T, int64_t c) {
  KsMvBufs b;
  b.part = ko_split_layout<float>(ar, B, M, N, c);
  b.ytmp = (T > 1 && !ks_mv_fused(T, c)) ? ar.take<float>((size_t)B * M * c) : nullptr;
  return b;
}

// the product on validated arguments
static int ksum_mv_run(const float* x1, const float* x2, const float* theta, unsigned fams, int T, int64_t B, int64_t M,
                       int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, KsMvBufs bufs,
                       const int* stop, hipStream_t st) {
  if (M != N) dmode = LO_DIAG_NONE;
  if (!ks_mv_fused(T, c)) {  // per term, left to right; the diagonal rides on the first term
    for (int t = 0; t < T; ++t) {
      int rc = kernel_mv_run(x1, x2, theta + (size_t)t * (D + 1), T * (D + 1), (int)((fams >> (4 * t)) & 15u), B, M, N, D,
                             v, c, d, t == 0 ? dmode : LO_DIAG_NONE, t == 0 ? y : bufs.ytmp, bufs.part, stop, st);
      if (!rc && t > 0) rc = vec_axpy1(y, bufs.ytmp, (size_t)B * M * c, stop, st);
      if (rc) return rc;
    }
    return LO_OK;
  }
  const KoSweep w(B, M, N, D);
  const size_t lds = ks_lds_bytes(T, w.DP, kKsCC);
  float* p = w.s.js > 1 ? bufs.part : nullptr;
  LO_PROF_BEGIN("k_ksum_mv", st);
  ko_pick(ko_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_ksum_mv<P(), kKsCC>), w.grid, dim3(kThreads), lds, st, x1, x2, theta, fams, T, (int)M, (int)N,
                       (int)D, v, (int)c, d, dmode, y, p, w.s.jchunk, stop);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (p)
    return ko_reduce_splits("k_ksum_mv_reduce", p, w.s.js, (size_t)M * c, (size_t)B * M * c, (int)c, d, dmode, v, y, stop,
                            st);
  return LO_OK;
}

// the layout of the derivative's workspace: the partials [T, DP + 1] of every workgroup
static float* ks_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D, int64_t T) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * s.rb * s.js * T * (ko_padded_dim(D) + 1));
}

int kernel_sum_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (!op.A0 || !op.A1 || op.R < 1 || !ks_terms_ok(op.nterms) || !ks_packed_ok(op.n2, op.nterms)) return LO_ERR_BADARG;
  if (!ko_shape_ok(op.B, op.N, op.N, op.R) || pl->c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  const KsMvBufs b = ks_mv_layout(*ar, op.B, op.N, op.N, op.nterms, pl->c);
  pl->ko.part = b.part;
  pl->ko.ytmp = b.ytmp;
  return LO_OK;
}

int kernel_sum_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  return ksum_mv_run(op.A0, op.A0, op.A1, (unsigned)op.n2, op.nterms, op.B, op.N, op.N, op.R, v, pl->c, op.d, op.diag_mode,
                     y, KsMvBufs{pl->ko.part, pl->ko.ytmp}, stop, st);
}

int kernel_sum_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->A1 || op->R < 1 || !ks_terms_ok(op->nterms) || !ks_packed_ok(op->n2, op->nterms)) return LO_ERR_BADARG;
  if (op->R > LO_KERNEL_MAX_DIM) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kernel_sum_mv_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t c) {
  if (!ko_args_ok(B, M, N, D, c) || !ks_terms_ok(T) || !ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ks_mv_layout(ar, B, M, N, T, c); });
}

int lo_kernel_sum_mv_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                         int64_t B, int64_t M, int64_t N, int64_t D, const float* v, int64_t c, const float* d,
                         int32_t diag_mode, float* y, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !families || !v || !y || !ko_args_ok(B, M, N, D, c) || !ks_terms_ok(T)) return LO_ERR_BADARG;
  const int64_t fams = ks_pack(families, T);
  if (fams < 0) return LO_ERR_BADARG;
  if (!ko_diag_ok(diag_mode, d, M == N)) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || c > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes, kKoTail);
  const KsMvBufs bufs = ks_mv_layout(ar, B, M, N, T, c);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  return ksum_mv_run(x1, x2, theta, (unsigned)fams, (int)T, B, M, N, D, v, c, d, diag_mode, y, bufs, nullptr,
                     (hipStream_t)stream);
}

size_t lo_kernel_sum_bilinear_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ks_terms_ok(T) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ks_bil_layout(ar, B, M, N, D, T); });
}

int lo_kernel_sum_bilinear_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                               int64_t B, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                               float* g_theta, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !families || !U || !V || !g_theta || !ko_args_ok(B, M, N, D, t) || !ks_terms_ok(T))
    return LO_ERR_BADARG;
  const int64_t fams = ks_pack(families, T);
  if (fams < 0) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ks_bil_layout(ar, B, M, N, D, T);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  const int TT = w.DP == 32 ? 2 : 4;  // (ks_bil_terms<DP>())
  for (int t0 = 0; t0 < (int)T; t0 += TT) {  // (one sweep unless 16 < D and T > 2)
    const int nt = std::min<int>(TT, (int)T - t0);
    const size_t lds = ks_lds_bytes(nt, w.DP, kKoTS);
    LO_PROF_BEGIN("k_ksum_bil", st);
    ko_pick(ko_dims{}, w.DP, [&](auto P) {
      hipLaunchKernelGGL((k_ksum_bil<P()>), w.grid, dim3(kThreads), lds, st, x1, x2, theta, (unsigned)fams, (int)T, t0, nt,
                         (int)M, (int)N, (int)D, U, V, (int)t, part, w.s.jchunk);
    });
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_ksum_bil_reduce, dim3((unsigned)B), dim3(kThreads), 0, st, part, w.s.rb * w.s.js, w.DP, (int)D,
                     (int)T, theta, g_theta);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

size_t lo_kernel_sum_points_grad_workspace_bytes(int64_t B, int64_t M, int64_t N, int64_t D, int64_t T, int64_t t) {
  if (!ko_args_ok(B, M, N, D, t) || !ks_terms_ok(T) || !ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return 0;
  return measured(kKoTail, [&](Arena& ar) { ko_split_layout<float>(ar, B, M, N, D); });
}

int lo_kernel_sum_points_grad_f32(const float* x1, const float* x2, const float* theta, const int32_t* families, int64_t T,
                                  int64_t B, int64_t M, int64_t N, int64_t D, const float* U, const float* V, int64_t t,
                                  float* g_x1, void* ws, size_t ws_bytes, void* stream) {
  if (!x1 || !x2 || !theta || !families || !U || !V || !g_x1 || !ko_args_ok(B, M, N, D, t) || !ks_terms_ok(T))
    return LO_ERR_BADARG;
  const int64_t fams = ks_pack(families, T);
  if (fams < 0) return LO_ERR_BADARG;
  if (!ko_shape_ok(B, M, N, D) || t > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kKoTail);
  float* part = ko_split_layout<float>(ar, B, M, N, D);  // [js, B, M, D]
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const KoSweep w(B, M, N, D);
  const size_t lds = ks_lds_bytes((int)T, w.DP, kKoTS);
  float* out = w.s.js > 1 ? part : g_x1;
  LO_PROF_BEGIN("k_ksum_pgrad", st);
  ko_pick(ko_dims{}, w.DP, [&](auto P) {
    hipLaunchKernelGGL((k_ksum_pgrad<P()>), w.grid, dim3(kThreads), lds, st, x1, x2, theta, (unsigned)fams, (int)T, (int)M,
                       (int)N, (int)D, U, V, (int)t, out, w.s.jchunk);
  });
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  if (w.s.js > 1)  // the splits in ascending order
    return ko_reduce_splits("k_ksum_pgrad_reduce", part, w.s.js, (size_t)M * D, (size_t)B * M * D, (int)D, nullptr,
                            LO_DIAG_NONE, nullptr, g_x1, nullptr, st);
  return LO_OK;
}

}  // extern "C"
