// lo_block.hip -- products of the block operators over a batch of B = G * T members (member g * T + t is block t of
// group g): BlockDiag, BlockInterleaved and SumBatch (reference: block_diag_linear_operator.py,
// block_interleaved_linear_operator.py, sum_batch_linear_operator.py over block_linear_operator.py:104-118).
//
// The reference reshapes the vectors to the batch of the base operator, multiplies, and reshapes back: for the
// interleaved row order (row i * T + t) that is a transposing copy in and out, and for the sum a [T, n, c] intermediate
// that is then reduced.  The kernels here read and write the vectors where they lie: the vector of member (g, t) is the
// strided view  v[g * gstride + i * ld + t * toff + k]  of the caller's tensor, and the sum over t runs inside the
// workgroup that owns the output rows (fixed order: results repeat bit for bit; no float atomics).
//   LO_BLOCK_DIAG         gstride T n c, ld c,   toff n c : the plain batched product (forwarded to lo_matvec_f32)
//   LO_BLOCK_INTERLEAVED  gstride n T c, ld T c, toff c
//   LO_BLOCK_SUM          gstride n c,   ld c,   toff 0   : every block reads the same vector, one output per group
// Dense members: one launch per chunk of up to 8 columns (k_blk_dense).  Low-rank members: partials of t = C^T v per
// row tile (k_blk_lr_tn), their sum in tile order (k_blk_lr_red), y = C t + d o v (k_blk_lr_nn).  Plain launches only.
#include <algorithm>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

struct BlkView {
  long long gstride, ld, toff;  // floats
  int T;                        // blocks per group
  int tl;                       // blocks summed into one output (SUM: T, else 1)
  int nt_out;                   // outputs per group and row (SUM: 1, else T)
};

static BlkView blk_view(int layout, int64_t T, int64_t n, int64_t c) {
  BlkView w;
  w.T = (int)T;
  if (layout == LO_BLOCK_SUM) {
    w.gstride = n * c, w.ld = c, w.toff = 0, w.tl = (int)T, w.nt_out = 1;
  } else if (layout == LO_BLOCK_INTERLEAVED) {
    w.gstride = n * T * c, w.ld = T * c, w.toff = c, w.tl = 1, w.nt_out = (int)T;
  } else {
    w.gstride = n * T * c, w.ld = c, w.toff = n * c, w.tl = 1, w.nt_out = (int)T;
  }
  return w;
}

// sum over the blocks an output row collects of their diagonal entries at `row`
__device__ __forceinline__ float blk_diag_sum(const float* __restrict__ dd, int dd_mode, long long m0, int tl, int n,
                                              int row) {
  float s = 0.f;
  if (dd_mode == LO_DIAG_FULL) {
    for (int tt = 0; tt < tl; ++tt) s += dd[(size_t)(m0 + tt) * n + row];
  } else if (dd_mode == LO_DIAG_CONST) {
    for (int tt = 0; tt < tl; ++tt) s += dd[m0 + tt];
  }
  return s;
}

// ---- dense members -------------------------------------------------------------------------------------------------
// One wave owns 4 rows at a time, its lanes stride over the columns of A (16 B per lane when VEC4), CT vector columns
// in registers; the t loop of LO_BLOCK_SUM runs around the column loop with the accumulators kept.
// grid (S * nt_out, G): blockIdx.x = s * nt_out + t, so that the workgroups that share the cache lines of the
// interleaved vectors (all t of one row range) are dispatched together.
constexpr int kBlkRB = 4;

template <int CT, bool VEC4>
__global__ __launch_bounds__(kThreads) void k_blk_dense(const float* __restrict__ A, const float* __restrict__ dd,
                                                         int dd_mode, const float* __restrict__ v,
                                                         float* __restrict__ y, BlkView w, int n, int cn,
                                                         int rows_per_wg) {
  const int s = blockIdx.x / w.nt_out, to = blockIdx.x % w.nt_out, g = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rows_per_wave = rows_per_wg / 4;
  const int wr0 = s * rows_per_wg + wave * rows_per_wave;
  const int wr1 = min(n, wr0 + rows_per_wave);
  const long long m0 = (long long)g * w.T + to;  // first member of this output (SUM: to == 0)
  const size_t voff = (size_t)g * w.gstride + (size_t)to * w.toff;
  const float* vb = v + voff;
  float* yb = y + voff;

  for (int row = wr0; row < wr1; row += kBlkRB) {
    float acc[kBlkRB][CT];
#pragma unroll
    for (int u = 0; u < kBlkRB; ++u)
#pragma unroll
      for (int k = 0; k < CT; ++k) acc[u][k] = 0.f;
    for (int tt = 0; tt < w.tl; ++tt) {
      const float* Am = A + (size_t)(m0 + tt) * n * n;
      const float* kr[kBlkRB];
#pragma unroll
      for (int u = 0; u < kBlkRB; ++u) kr[u] = Am + (size_t)min(row + u, n - 1) * n;
      if (VEC4) {
        for (int j = 4 * lane; j < n; j += 256) {  // (n % 4 == 0)
          float4 a[kBlkRB];
#pragma unroll
          for (int u = 0; u < kBlkRB; ++u) a[u] = *reinterpret_cast<const float4*>(kr[u] + j);
          float vv[4][CT];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int k = 0; k < CT; ++k) vv[jj][k] = (k < cn) ? vb[(size_t)(j + jj) * w.ld + k] : 0.f;
#pragma unroll
          for (int u = 0; u < kBlkRB; ++u)
#pragma unroll
            for (int k = 0; k < CT; ++k) {
              float t = acc[u][k];
              t = fmaf(a[u].x, vv[0][k], t);
              t = fmaf(a[u].y, vv[1][k], t);
              t = fmaf(a[u].z, vv[2][k], t);
              t = fmaf(a[u].w, vv[3][k], t);
              acc[u][k] = t;
            }
        }
      } else {
        for (int j = lane; j < n; j += 64) {
          float vv[CT];
#pragma unroll
          for (int k = 0; k < CT; ++k) vv[k] = (k < cn) ? vb[(size_t)j * w.ld + k] : 0.f;
#pragma unroll
          for (int u = 0; u < kBlkRB; ++u) {
            const float a = kr[u][j];
#pragma unroll
            for (int k = 0; k < CT; ++k) acc[u][k] = fmaf(a, vv[k], acc[u][k]);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kBlkRB; ++u)
#pragma unroll
      for (int k = 0; k < CT; ++k) acc[u][k] = wave_sum(acc[u][k]);
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < kBlkRB; ++u) {
        const int rr = row + u;
        if (rr < wr1) {
          const float dv = blk_diag_sum(dd, dd_mode, m0, w.tl, n, rr);
#pragma unroll
          for (int k = 0; k < CT; ++k)
            if (k < cn) yb[(size_t)rr * w.ld + k] = fmaf(dv, vb[(size_t)rr * w.ld + k], acc[u][k]);
        }
      }
    }
  }
}

static int blk_rows_per_wg(int64_t wgs_per_tile, int64_t n) {
  int64_t rows = 128;  // >= ~1024 workgroups when possible, 16 .. 128 rows per workgroup
  while (rows > 16 && wgs_per_tile * ((n + rows - 1) / rows) < 1024) rows /= 2;
  return (int)rows;
}

static int blk_dense_run(const lo_op_desc* op, const BlkView& w, int64_t G, const float* v, float* y, int64_t c,
                         hipStream_t st) {
  const int n = (int)op->N;
  const int rows = blk_rows_per_wg(G * w.nt_out, n);
  const int64_t S = (n + rows - 1) / rows;
  if (S * w.nt_out > 0x7fffffffLL || G > 65535) return LO_ERR_UNSUPPORTED;
  const bool vec4 = (n % 4 == 0) && ((uintptr_t)op->A0 % 16 == 0);
  dim3 grid((unsigned)(S * w.nt_out), (unsigned)G), block(kThreads);
  for (int64_t c0 = 0; c0 < c;) {
    const int left = (int)std::min<int64_t>(8, c - c0);
    const int ct = left >= 8 ? 8 : left >= 4 ? 4 : left >= 2 ? 2 : 1;
#define LO_BD(CT, V4)                                                                                          \
  hipLaunchKernelGGL((k_blk_dense<CT, V4>), grid, block, 0, st, op->A0, op->d, op->diag_mode, v + c0, y + c0, w, n, \
                     ct, rows)
    LO_PROF_BEGIN("k_blk_dense", st);
    if (vec4) {
      if (ct == 8) LO_BD(8, true);
      else if (ct == 4) LO_BD(4, true);
      else if (ct == 2) LO_BD(2, true);
      else LO_BD(1, true);
    } else {
      if (ct == 8) LO_BD(8, false);
      else if (ct == 4) LO_BD(4, false);
      else if (ct == 2) LO_BD(2, false);
      else LO_BD(1, false);
    }
#undef LO_BD
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
    c0 += ct;
  }
  return LO_OK;
}

// ---- low-rank members: y = C (C^T v) + d o v -------------------------------------------------------------------------
constexpr int kBlkTile = 32;   // rows staged in LDS at a time
constexpr int kBlkAcc = 8;     // outputs a thread of k_blk_lr_tn keeps: R * cn <= 2048 per column chunk
constexpr int kBlkAccNN = 4;   // outputs a thread of k_blk_lr_nn keeps: kBlkTile * cn <= 1024
constexpr int kBlkMaxChunk = 32;  // columns per chunk (both kernels; with R * cn <= 2048 the LDS of either stays below 48 KiB)

static int blk_lr_chunk(int64_t R, int64_t c) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(c, kBlkMaxChunk), (kBlkAcc * kThreads) / R));
}

// tpart[m, s, r, k] = sum over the rows i of tile s of C_m[i, r] v_m[i, k]; grid (S * T, G), blockIdx.x = s * T + t.
// LDS: Cs [kBlkTile, R], vs [kBlkTile, cn].
__global__ __launch_bounds__(kThreads) void k_blk_lr_tn(const float* __restrict__ Cr, const float* __restrict__ v,
                                                         float* __restrict__ tpart, BlkView w, int n, int R, int c,
                                                         int chunk, int rows_per_wg, int S, int vec4) {
  extern __shared__ float4 blk_smem4[];
  float* Cs = reinterpret_cast<float*>(blk_smem4);
  float* vs = Cs + (size_t)kBlkTile * R;
  const int s = blockIdx.x / w.T, t = blockIdx.x % w.T, g = blockIdx.y;
  const long long m = (long long)g * w.T + t;
  const int r0 = s * rows_per_wg, r1 = min(n, r0 + rows_per_wg);
  const float* Cm = Cr + (size_t)m * n * R;
  const float* vb = v + (size_t)g * w.gstride + (size_t)t * w.toff;
  float* out = tpart + ((size_t)m * S + s) * R * c;
  for (int c0 = 0; c0 < c; c0 += chunk) {
    const int cn = min(chunk, c - c0);
    const int E = R * cn;
    float acc[kBlkAcc];
#pragma unroll
    for (int q = 0; q < kBlkAcc; ++q) acc[q] = 0.f;
    for (int i0 = r0; i0 < r1; i0 += kBlkTile) {
      const int ni = min(kBlkTile, r1 - i0);
      __syncthreads();
      const float* src = Cm + (size_t)i0 * R;
      if (vec4) {  // (R % 4 == 0 and a 16-byte aligned C)
        for (int idx = threadIdx.x; idx < ni * R / 4; idx += kThreads)
          reinterpret_cast<float4*>(Cs)[idx] = reinterpret_cast<const float4*>(src)[idx];
      } else {
        for (int idx = threadIdx.x; idx < ni * R; idx += kThreads) Cs[idx] = src[idx];
      }
      for (int idx = threadIdx.x; idx < ni * cn; idx += kThreads) {
        const int i = idx / cn, k = idx % cn;
        vs[idx] = vb[(size_t)(i0 + i) * w.ld + c0 + k];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBlkAcc; ++q) {
        const int e = threadIdx.x + q * kThreads;
        if (e < E) {
          const int r = e / cn, k = e % cn;
          float a = acc[q];
          for (int i = 0; i < ni; ++i) a = fmaf(Cs[i * R + r], vs[i * cn + k], a);
          acc[q] = a;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kBlkAcc; ++q) {
      const int e = threadIdx.x + q * kThreads;
      if (e < E) out[(size_t)(e / cn) * c + c0 + e % cn] = acc[q];
    }
  }
}

// tsum[m, e] = sum_s tpart[m, s, e] in tile order (e over R * c)
__global__ __launch_bounds__(kThreads) void k_blk_lr_red(const float* __restrict__ tpart, float* __restrict__ tsum,
                                                          long long per_member, int S, long long total) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const long long m = idx / per_member, e = idx % per_member;
  const float* p = tpart + (size_t)m * S * per_member + e;
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += p[(size_t)s * per_member];
  tsum[idx] = a;
}

// y[g, i, (t,) k] = sum over the blocks of this output of C_m[i, :] tsum[m, :, k]  +  (sum of their d[i]) v[i, k]
// grid (S2 * nt_out, G); a workgroup owns kBlkTile rows.  LDS: Cs [kBlkTile, R + 1], ts [R, cn].
__global__ __launch_bounds__(kThreads) void k_blk_lr_nn(const float* __restrict__ Cr, const float* __restrict__ tsum,
                                                         const float* __restrict__ dd, int dd_mode,
                                                         const float* __restrict__ v, float* __restrict__ y, BlkView w,
                                                         int n, int R, int c, int chunk) {
  extern __shared__ float4 blk_smem4[];
  float* Cs = reinterpret_cast<float*>(blk_smem4);
  float* ts = Cs + (size_t)kBlkTile * (R + 1);
  const int s = blockIdx.x / w.nt_out, to = blockIdx.x % w.nt_out, g = blockIdx.y;
  const long long m0 = (long long)g * w.T + to;
  const int i0 = s * kBlkTile, ni = min(kBlkTile, n - i0);
  const size_t voff = (size_t)g * w.gstride + (size_t)to * w.toff;
  const float* vb = v + voff;
  float* yb = y + voff;
  for (int c0 = 0; c0 < c; c0 += chunk) {
    const int cn = min(chunk, c - c0);
    const int E = ni * cn;
    float acc[kBlkAccNN];
#pragma unroll
    for (int q = 0; q < kBlkAccNN; ++q) acc[q] = 0.f;
    for (int tt = 0; tt < w.tl; ++tt) {
      const long long m = m0 + tt;
      __syncthreads();
      if (tt == 0 && c0 > 0 && w.tl == 1) {
        // (one block per output: its rows of C are staged already)
      } else {
        const float* src = Cr + ((size_t)m * n + i0) * R;
        for (int idx = threadIdx.x; idx < ni * R; idx += kThreads) Cs[(idx / R) * (R + 1) + idx % R] = src[idx];
      }
      for (int idx = threadIdx.x; idx < R * cn; idx += kThreads)
        ts[idx] = tsum[(size_t)m * R * c + (size_t)(idx / cn) * c + c0 + idx % cn];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBlkAccNN; ++q) {
        const int e = threadIdx.x + q * kThreads;
        if (e < E) {
          const int i = e / cn, k = e % cn;
          float a = acc[q];
          for (int r = 0; r < R; ++r) a = fmaf(Cs[i * (R + 1) + r], ts[r * cn + k], a);
          acc[q] = a;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kBlkAccNN; ++q) {
      const int e = threadIdx.x + q * kThreads;
      if (e < E) {
        const int i = e / cn, k = e % cn;
        const size_t at = (size_t)(i0 + i) * w.ld + c0 + k;
        const float dv = blk_diag_sum(dd, dd_mode, m0, w.tl, n, i0 + i);
        yb[at] = fmaf(dv, vb[at], acc[q]);
      }
    }
  }
}

static int blk_lr_rows_per_wg(int64_t B, int64_t n) {
  int64_t rows = 256;  // >= ~512 workgroups when possible, a multiple of the staged tile
  while (rows > kBlkTile && B * ((n + rows - 1) / rows) < 512) rows /= 2;
  return (int)rows;
}

static size_t blk_lr_bytes(const lo_op_desc* op, int64_t c) {
  const int rows = blk_lr_rows_per_wg(op->B, op->N);
  const int64_t S = (op->N + rows - 1) / rows;
  Arena ar(nullptr, 0);
  ar.take<float>((size_t)op->B * S * op->R * c);
  ar.take<float>((size_t)op->B * op->R * c);
  return ar.off + 256;
}

static int blk_lr_run(const lo_op_desc* op, const BlkView& w, int64_t G, const float* v, float* y, int64_t c, void* ws,
                      size_t ws_bytes, hipStream_t st) {
  const int n = (int)op->N, R = (int)op->R;
  if (!ws) return LO_ERR_WORKSPACE;
  const int rows = blk_lr_rows_per_wg(op->B, n);
  const int64_t S = (n + rows - 1) / rows, S2 = (n + kBlkTile - 1) / kBlkTile;
  if (S * w.T > 0x7fffffffLL || S2 * w.nt_out > 0x7fffffffLL || G > 65535 || c > 0x7fffffffLL / R)
    return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes);
  float* tpart = ar.take<float>((size_t)op->B * S * R * c);
  float* tsum = ar.take<float>((size_t)op->B * R * c);
  if (!ar.ok) return LO_ERR_WORKSPACE;
  const int chunk = blk_lr_chunk(R, c);
  const int vec4 = (R % 4 == 0) && ((uintptr_t)op->A0 % 16 == 0);
  {
    dim3 grid((unsigned)(S * w.T), (unsigned)G), block(kThreads);
    const size_t lds = ((size_t)kBlkTile * R + (size_t)kBlkTile * chunk) * sizeof(float);
    LO_PROF_BEGIN("k_blk_lr_tn", st);
    hipLaunchKernelGGL(k_blk_lr_tn, grid, block, lds, st, op->A0, v, tpart, w, n, R, (int)c, chunk, rows, (int)S, vec4);
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
  }
  {
    const long long per_member = (long long)R * c, total = per_member * op->B;
    const long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return LO_ERR_UNSUPPORTED;
    LO_PROF_BEGIN("k_blk_lr_red", st);
    hipLaunchKernelGGL(k_blk_lr_red, dim3((unsigned)blocks), dim3(kThreads), 0, st, tpart, tsum, per_member, (int)S,
                       total);
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
  }
  {
    dim3 grid((unsigned)(S2 * w.nt_out), (unsigned)G), block(kThreads);
    const size_t lds = ((size_t)kBlkTile * (R + 1) + (size_t)R * chunk) * sizeof(float);
    LO_PROF_BEGIN("k_blk_lr_nn", st);
    hipLaunchKernelGGL(k_blk_lr_nn, grid, block, lds, st, op->A0, tsum, op->d, op->diag_mode, v, y, w, n, R, (int)c,
                       chunk);
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
  }
  return LO_OK;
}

static int blk_check(const lo_op_desc* op, int32_t layout, int64_t T, int64_t c) {
  if (!op || T < 1 || c < 1 || op->B < 1 || op->N < 1) return LO_ERR_BADARG;
  if (layout != LO_BLOCK_DIAG && layout != LO_BLOCK_INTERLEAVED && layout != LO_BLOCK_SUM) return LO_ERR_BADARG;
  if (op->kind != LO_OP_DENSE_DIAG && op->kind != LO_OP_LOWRANK_DIAG) return LO_ERR_UNSUPPORTED;
  if (op->B % T != 0) return LO_ERR_BADARG;
  if (op->diag_mode != LO_DIAG_NONE && op->diag_mode != LO_DIAG_FULL && op->diag_mode != LO_DIAG_CONST)
    return LO_ERR_BADARG;
  if (!op->A0 || (op->diag_mode != LO_DIAG_NONE && !op->d)) return LO_ERR_BADARG;
  if (op->kind == LO_OP_LOWRANK_DIAG && op->R < 1) return LO_ERR_BADARG;
  if (op->kind == LO_OP_LOWRANK_DIAG && op->R > kMaxRank) return LO_ERR_UNSUPPORTED;
  if (op->N > 0x7fffffffLL / 2 || T > 0x7fffffffLL / 2) return LO_ERR_UNSUPPORTED;
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_block_mv_workspace_bytes(const lo_op_desc* base, int32_t layout, int64_t T, int64_t c) {
  if (blk_check(base, layout, T, c) != LO_OK) return 0;
  if (layout == LO_BLOCK_DIAG) return lo_matvec_workspace_bytes(base, c);
  return base->kind == LO_OP_LOWRANK_DIAG ? blk_lr_bytes(base, c) : 256;
}

int lo_block_mv_f32(const lo_op_desc* base, int32_t layout, int64_t T, const float* v, float* y, int64_t c, void* ws,
                    size_t ws_bytes, void* stream) {
  const int rc = blk_check(base, layout, T, c);
  if (rc) return rc;
  if (!v || !y) return LO_ERR_BADARG;
  if (layout == LO_BLOCK_DIAG) return lo_matvec_f32(base, v, y, c, ws, ws_bytes, stream);
  hipStream_t st = (hipStream_t)stream;
  const BlkView w = blk_view(layout, T, base->N, c);
  const int64_t G = base->B / T;
  if (base->kind == LO_OP_DENSE_DIAG) return blk_dense_run(base, w, G, v, y, c, st);
  return blk_lr_run(base, w, G, v, y, c, ws, ws_bytes, st);
}

}  // extern "C"
