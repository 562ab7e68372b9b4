// lo_ski_grid.hip -- SKI on a 2-D / 3-D grid: the base of the interpolated operator is a Kronecker product of D symmetric
// Toeplitz matrices, one per grid axis (GridInterpolationKernel on multi-dimensional inputs).
//   KroneckerProductLinearOperator._matmul (kronecker_product_linear_operator.py:272-284) over
//   ToeplitzLinearOperator._matmul         (toeplitz_linear_operator.py:42-53)
//
// The grid vector is u [B, M_1, .., M_D, c], row-major, columns fastest: the [B, M, c] layout of the interpolation
// kernels of lo_ski.hip with the grid index g = (g_1 M_2 + g_2) M_3 + g_3.  (T_1 (x) .. (x) T_D) u is applied one axis
// per pass.  For axis k the vector is viewed as [lines = B * outer, M_k, inner], inner = (prod_{j > k} M_j) c, and
//   y[l, i, s] = sum_j t_k[|i - j|] u[l, j, s],   j ascending.
// No M_k x M_k matrix exists: the lags of a member are staged in LDS as the mirrored window win[x] = t_k[|x - off|], so
// that the lag of (i, j) is read at win[i - j + off] without an absolute value in the loop.  One workgroup owns the whole
// sum of its outputs (M_k <= LO_SKI_GRID_MAX_AXIS: no split over j, no partials), sums run in ascending j: the same
// inputs give the same bits.
//
// Two lane mappings, chosen from the shape alone:
//   k_grid_axis_inner  inner >= 64: the 64 lanes of a wave run along `inner` (coalesced rows of u and y), the four waves
//                      of a workgroup take different output rows i, RI rows per thread.  A [64 j x 64 s] tile of u is
//                      staged in LDS and shared by the four waves; the lags of a wave are wave-uniform (LDS broadcast
//                      reads), 2 RI - 1 of them serve RI x RI products.
//   k_grid_axis_line   inner < 64 (the last axis with few columns): a thread per output element of a line [M_k, inner],
//                      consecutive threads on consecutive elements (i, s) -- lanes run along i -- with the line staged
//                      in LDS in chunks of j.  The reads of the line are broadcasts of at most `inner` consecutive
//                      addresses, the reads of the window consecutive addresses: no bank conflicts.  Lines shorter than
//                      a workgroup share one.
//
// The same passes alone are the kind LO_OP_TOEPLITZ_KRON_DIAG (the base operator without interpolation: a GP whose data
// lie on the grid), with the + d o v term in the store of the last pass, and the first half of the column gradients
// lo_toeplitz_kron_bilinear_f32 (k_grid_axis_corr below).
#include <algorithm>
#include <cstdlib>
#include <climits>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

constexpr int kGridMaxAxis = LO_SKI_GRID_MAX_AXIS;
constexpr int kGridPad = 64;                                // j runs to the next multiple of 64 in k_grid_axis_inner
constexpr int kGridWin = 2 * kGridMaxAxis + 2 * kGridPad;   // mirrored lag window (+ the rows / j beyond M_k)
constexpr int kGridTile = 64;                               // j tile and s tile of k_grid_axis_inner
constexpr int kGridStage = 4096;                            // floats of a line chunk in k_grid_axis_line

// The + d o v term of a pass that writes an operator's result (the last pass of LO_OP_TOEPLITZ_KRON_DIAG, where
// inner == c and element e of the grid vector belongs to row e / inner of d); mode LO_DIAG_NONE: nothing is added.
struct GridDiag {
  const float* d;
  int mode;
  const float* v;
};

__device__ __forceinline__ float grid_add_diag(const GridDiag& dg, float acc, size_t b, size_t e, int64_t inner) {
  if (dg.mode == LO_DIAG_FULL) return fmaf(dg.d[e / inner], dg.v[e], acc);
  if (dg.mode == LO_DIAG_CONST) return fmaf(dg.d[b], dg.v[e], acc);
  return acc;
}

// win[x] = t[|x - off|] where that lag exists, else 0
__device__ __forceinline__ void grid_stage_window(const float* __restrict__ t, int M, int off, int n, float* win) {
  for (int x = threadIdx.x; x < n; x += kThreads) {
    const int d = x - off;
    const int ad = d < 0 ? -d : d;
    win[x] = ad < M ? t[ad] : 0.f;
  }
}

// blockIdx.x = (line, i tile, s tile), s tile fastest
template <int RI>
__global__ __launch_bounds__(kThreads) void k_grid_axis_inner(const float* __restrict__ t, int64_t tstride, int M,
                                                               int64_t outer, int64_t inner, int stiles, int itiles,
                                                               const float* __restrict__ u, float* __restrict__ y,
                                                               GridDiag dg, const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ float us[kGridTile * kGridTile];
  __shared__ float win[kGridWin];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t blk = blockIdx.x;
  const int st = (int)(blk % stiles);
  const int it = (int)((blk / stiles) % itiles);
  const size_t line = blk / ((size_t)stiles * itiles);
  const size_t b = line / outer;
  const int64_t s = (int64_t)st * kGridTile + lane;
  const bool s_ok = s < inner;
  const int i0 = (it * 4 + wave) * RI;  // first output row of this wave
  const int off = M - 1 + kGridPad;
  const float* ul = u + line * (size_t)M * inner;
  float* yl = y + line * (size_t)M * inner;
  grid_stage_window(t + b * tstride, M, off, 2 * M - 1 + 2 * kGridPad, win);
  float acc[RI];
#pragma unroll
  for (int r = 0; r < RI; ++r) acc[r] = 0.f;
  for (int j0 = 0; j0 < M; j0 += kGridTile) {
    __syncthreads();
#pragma unroll 4
    for (int jj = wave; jj < kGridTile; jj += 4) {
      const int j = j0 + jj;
      us[jj * kGridTile + lane] = (j < M && s_ok) ? ul[(size_t)j * inner + s] : 0.f;
    }
    __syncthreads();
    // lag of (row i0 + r, column j0 + jb + q) at w[r - q]; per block of RI columns the 2 RI - 1 lags wl[x] = w[x - (RI - 1)]
    for (int jb = 0; jb < kGridTile; jb += RI) {
      const float* w = win + (i0 - (j0 + jb) + off);
      float wl[2 * RI - 1];
#pragma unroll
      for (int x = 0; x < 2 * RI - 1; ++x) wl[x] = w[x - (RI - 1)];
#pragma unroll
      for (int q = 0; q < RI; ++q) {
        const float uv = us[(jb + q) * kGridTile + lane];
#pragma unroll
        for (int r = 0; r < RI; ++r) acc[r] = fmaf(wl[r - q + RI - 1], uv, acc[r]);
      }
    }
  }
  if (s_ok) {
#pragma unroll
    for (int r = 0; r < RI; ++r)
      if (i0 + r < M) {
        const size_t e = (size_t)(i0 + r) * inner + s;
        yl[e] = grid_add_diag(dg, acc[r], b, line * (size_t)M * inner + e, inner);
      }
  }
}

// blockIdx.x = (line group, block of the line), block of the line fastest; lpb lines per workgroup (LS < 256) or
// bpl workgroups per line
__global__ __launch_bounds__(kThreads) void k_grid_axis_line(const float* __restrict__ t, int64_t tstride, int M,
                                                              int64_t outer, int inner, int64_t lines, int lpb, int bpl,
                                                              int jc, const float* __restrict__ u,
                                                              float* __restrict__ y, GridDiag dg,
                                                              const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ float ls[kGridStage];
  __shared__ float win[kGridWin];
  const int LS = M * inner;  // floats of a line (<= 1024 * 63)
  const size_t grp = blockIdx.x / bpl;
  const int lb = (int)(blockIdx.x % bpl);
  const size_t line0 = grp * lpb;
  const int nl = (int)std::min<int64_t>(lpb, lines - (int64_t)line0);  // lines of this workgroup
  // (the window is per member: the host keeps the lines of a workgroup inside one member -- lpb divides outer)
  const size_t b = line0 / outer;
  const int off = M - 1;
  grid_stage_window(t + b * tstride, M, off, 2 * M - 1, win);
  const int e = lb * kThreads + threadIdx.x;  // element of the workgroup's lines
  const int ll = e / LS;                     // line within the group
  const int el = e - ll * LS;
  const int i = el / inner, s = el - i * inner;
  const bool live = ll < nl;
  const float* ug = u + line0 * (size_t)LS;
  float acc = 0.f;
  for (int j0 = 0; j0 < M; j0 += jc) {
    const int nj = min(jc, M - j0);
    __syncthreads();
    // rows j0 .. j0 + nj of every line of the group: [nl][nj * inner], contiguous per line
    const int per = nj * inner;
    for (int x = threadIdx.x; x < nl * per; x += kThreads) {
      const int l = x / per, r = x - l * per;
      ls[x] = ug[(size_t)l * LS + (size_t)j0 * inner + r];
    }
    __syncthreads();
    if (live) {
      const float* lp = ls + ll * per + s;
      const float* w = win + (i - j0 + off);
#pragma unroll 4
      for (int jj = 0; jj < nj; ++jj) acc = fmaf(w[-jj], lp[jj * inner], acc);
    }
  }
  if (live) y[line0 * (size_t)LS + e] = grid_add_diag(dg, acc, b, line0 * (size_t)LS + e, inner);
}

static bool grid_shape_ok(const int64_t* m, int ndim, int64_t* M_out) {
  if (ndim != 2 && ndim != 3) return false;
  int64_t M = 1;
  for (int k = 0; k < ndim; ++k) {
    if (m[k] < 1 || m[k] > kGridMaxAxis) return false;
    M *= m[k];
  }
  if (M > LO_SKI_GRID_MAX_M) return false;
  *M_out = M;
  return true;
}

// one axis: y = (I (x) T_k (x) I) u on [B * outer, Mk, inner]
static int grid_axis(const float* t, int64_t tstride, int64_t B, int64_t outer, int64_t Mk, int64_t inner, const float* u,
                     float* y, const GridDiag& dg, const int* stop, hipStream_t st) {
  const int64_t lines = B * outer;
  if (inner >= 64) {
    const int64_t stiles = (inner + kGridTile - 1) / kGridTile;
    // 8 rows per thread when that still fills the device, else 2 (a function of the shape only)
    const bool big = lines * stiles * ((Mk + 31) / 32) >= 512;
    const int rows = big ? 32 : 8;
    const int64_t itiles = (Mk + rows - 1) / rows;
    const int64_t nblk = lines * stiles * itiles;
    if (stiles > INT_MAX || nblk > INT_MAX) return LO_ERR_UNSUPPORTED;
    if (big)
      hipLaunchKernelGGL((k_grid_axis_inner<8>), dim3((unsigned)nblk), dim3(kThreads), 0, st, t, tstride, (int)Mk, outer,
                         inner, (int)stiles, (int)itiles, u, y, dg, stop);
    else
      hipLaunchKernelGGL((k_grid_axis_inner<2>), dim3((unsigned)nblk), dim3(kThreads), 0, st, t, tstride, (int)Mk, outer,
                         inner, (int)stiles, (int)itiles, u, y, dg, stop);
  } else {
    const int64_t LS = Mk * inner;
    int lpb = 1, bpl = 1, jc = (int)Mk;
    if (LS >= kThreads) {
      bpl = (int)((LS + kThreads - 1) / kThreads);
      jc = (int)std::min<int64_t>(Mk, kGridStage / inner);
    } else {
      // several lines per workgroup, all of one member: the largest divisor of `outer` not above 256 / LS
      lpb = (int)std::min<int64_t>(kThreads / LS, outer);
      while (outer % lpb) --lpb;
    }
    const int64_t nblk = (lines + lpb - 1) / lpb * bpl;
    if (nblk > INT_MAX) return LO_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k_grid_axis_line, dim3((unsigned)nblk), dim3(kThreads), 0, st, t, tstride, (int)Mk, outer,
                       (int)inner, lines, lpb, bpl, jc, u, y, dg, stop);
  }
  return LO_OK;
}

size_t toeplitz_kron_ws_bytes(int64_t B, int64_t M, int64_t c) {
  return align_up((size_t)B * M * c * sizeof(float), 256) + 256;
}

// D passes, axis 1 first, ping-pong between the two grid vectors buf0 / buf1: the passes read src, buf1, buf0 and write
// buf1, buf0, buf1, so the result is in buf0 (D = 2) or buf1 (D = 3), returned through *out.  src may be buf0 itself
// (it is consumed by the first pass before the second overwrites it) or a read-only input.  `dg` (or nullptr): the
// diagonal term added in the store of the last pass.
int toeplitz_kron_passes(const float* t, const int64_t* m, int ndim, int64_t B, int64_t c, const float* src, float* buf0,
                         float* buf1, float** out, const int* stop, hipStream_t st, const GridDiag* dg = nullptr) {
  int64_t M = 1, sumM = 0;
  for (int k = 0; k < ndim; ++k) {
    M *= m[k];
    sumM += m[k];
  }
  const float* in = src;
  float* bufs[2] = {buf1, buf0};
  int64_t outer = 1, toff = 0;
  LO_PROF_BEGIN("ski_grid_mv", st);
  for (int k = 0; k < ndim; ++k) {
    const int64_t inner = M / (outer * m[k]) * c;
    float* dst = bufs[k & 1];
    const GridDiag none{nullptr, LO_DIAG_NONE, nullptr};
    const int rc = grid_axis(t + toff, sumM, B, outer, m[k], inner, in, dst, (dg && k == ndim - 1) ? *dg : none, stop, st);
    if (rc) {
      LO_PROF_END(st);
      return rc;
    }
    in = dst;
    outer *= m[k];
    toff += m[k];
  }
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  *out = bufs[(ndim - 1) & 1];
  return LO_OK;
}

// ---- the kind's plan and run functions (lo_matvec.hip): those of lo_ski.hip with the Toeplitz product replaced ------
int ski_grid_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !interp_ptrs_ok(op->interp)) return LO_ERR_BADARG;
  int64_t M = 0;
  if (!grid_shape_ok(op->interp->grid_m, op->interp->grid_ndim, &M)) return LO_ERR_UNSUPPORTED;
  return M != op->R ? LO_ERR_BADARG : LO_OK;
}

int ski_grid_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  if (const int rc = ski_grid_desc_check(&op)) return rc;
  if (!interp_shape_ok(op.B, op.N, op.n2, op.R) || pl->c > INT_MAX / 64) return LO_ERR_BADARG;  // (32-bit limits)
  return ski_interp_plan(pl, op.R, ar, st);
}

int ski_grid_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const SkiPlan& k = pl->ski;
  const int64_t M = op.R;
  int rc = interp_scatter(k.csr.ptr, k.csr.ids, k.w.right_vals, op.B, op.N, op.n2, M, v, pl->c, k.u, stop, st);
  float* g = nullptr;  // the passes write t, u, t: the result is in u (D = 2) or t (D = 3)
  if (!rc) rc = toeplitz_kron_passes(op.A0, k.w.grid_m, k.w.grid_ndim, op.B, pl->c, k.u, k.u, k.t, &g, stop, st);
  if (!rc) rc = interp_gather(k.w.left_idx, k.w.left_vals, op.B, op.N, op.n2, M, g, pl->c, op.d, op.diag_mode, v, y,
                              stop, st);
  return rc;
}

// ---- LO_OP_TOEPLITZ_KRON_DIAG: y = (T_1 (x) .. (x) T_D) v + d o v ---------------------------------------------------------
int toeplitz_kron_desc_check(const lo_op_desc* op) {
  if (!op->A0 || !op->grid) return LO_ERR_BADARG;
  int64_t M = 0;
  if (!grid_shape_ok(op->grid->m, op->grid->ndim, &M)) return LO_ERR_UNSUPPORTED;
  return (M != op->N || M != op->R) ? LO_ERR_BADARG : LO_OK;
}

int toeplitz_kron_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  if (const int rc = toeplitz_kron_desc_check(&op)) return rc;
  if (pl->c > INT_MAX / 64) return LO_ERR_BADARG;
  pl->tk.g = *op.grid;
  pl->tk.tmp = ar->take<float>((size_t)op.B * op.N * pl->c);
  // A/B switch of DESIGN.md section 6j: the diagonal as vec_add_diag behind the passes instead of in the last store
  pl->tk.epilogue = getenv("LO_TKRON_EPILOGUE") != nullptr;
  return LO_OK;
}

int toeplitz_kron_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const ToeplitzKronPlan& k = pl->tk;
  const bool has_diag = op.diag_mode != LO_DIAG_NONE;
  const GridDiag dg{op.d, op.diag_mode, v};
  const GridDiag* fused = (has_diag && !k.epilogue) ? &dg : nullptr;
  // v -> tmp -> y (D = 2), v -> y -> tmp -> y (D = 3): the last pass writes y
  float* out = nullptr;
  int rc = k.g.ndim == 2 ? toeplitz_kron_passes(op.A0, k.g.m, 2, op.B, pl->c, v, y, k.tmp, &out, stop, st, fused)
                         : toeplitz_kron_passes(op.A0, k.g.m, 3, op.B, pl->c, v, k.tmp, y, &out, stop, st, fused);
  if (!rc && has_diag && !fused) rc = vec_add_diag(op.d, op.diag_mode, v, y, pl->c, op.B, op.N, pl->sp, stop, st);
  return rc;
}

// ---- column gradients: the axis lag correlation ------------------------------------------------------------------------
// p, q [lines = B * outer, Mk, inner]:  part[chunk, b, l] = sum over the chunk's (line of b, s tile) units, s, i of
//   p[i, s] q[i + l, s] + [l > 0] p[i + l, s] q[i, s]
// -- k_tz_bil of lo_ski.hip for many strided lines.  Lanes run along the lag l (256 lags per workgroup).  A tile of
// kCorrI rows i x ts <= kCorrS columns s of p and q and the windows [i0 + l0, i0 + l0 + kCorrI + 256) of both are staged
// in LDS with s outermost: the window read q[s][x + lane] touches consecutive addresses, p[s][x] is a broadcast.  The row
// stride of the window is odd, so that the staging writes of one row's columns (stride = row stride) fall into
// different banks (the tile rows likewise): 16 * (2 * 65 + 2 * 321) floats = 48 KiB of LDS.
// A tile whose every product lies beyond the axis (i0 + l0 >= Mk) is skipped, as are the rows of a tile and of a window
// beyond it and the waves whose lags all are.  Units are handed out in contiguous
// chunks, a function of the shape alone; the partials are added by k_grid_corr_reduce in ascending chunk order.
constexpr int kCorrI = 64;
constexpr int kCorrS = 16;
constexpr int kCorrA = kCorrI + 1;             // tile row stride (odd)
constexpr int kCorrW = kCorrI + kThreads + 1;  // window row stride (odd)

// grid (lag block, chunk, member)
__global__ __launch_bounds__(kThreads) void k_grid_axis_corr(const float* __restrict__ p, const float* __restrict__ q,
                                                              int Mk, int64_t outer, int64_t inner, int stiles,
                                                              int64_t units, int64_t per_chunk,
                                                              float* __restrict__ part) {
  __shared__ float pa[kCorrS * kCorrA], qa[kCorrS * kCorrA], pw[kCorrS * kCorrW], qw[kCorrS * kCorrW];
  const int l0 = blockIdx.x * kThreads;
  const int l = l0 + threadIdx.x;
  const bool wave_live = l0 + (int)(threadIdx.x & ~63u) < Mk;  // (lanes beyond Mk of a live wave read unstaged rows: never stored)
  const size_t chunk = blockIdx.y, b = blockIdx.z, B = gridDim.z;
  const int64_t u0 = (int64_t)chunk * per_chunk, u1 = min(units, u0 + per_chunk);
  float a1 = 0.f, a2 = 0.f;
  for (int64_t un = u0; un < u1; ++un) {
    const int64_t o = un / stiles;
    const int64_t s0 = (un - o * stiles) * kCorrS;
    const int ts = (int)min((int64_t)kCorrS, inner - s0);
    const size_t base = (b * outer + o) * (size_t)Mk * inner + s0;
    for (int i0 = 0; i0 + l0 < Mk; i0 += kCorrI) {
      const int nx = min(kCorrI, Mk - i0);                  // rows of the tile inside the axis
      const int nw = min(kCorrI + kThreads, nx + Mk - l0);  // window rows a stored lag can read (zero beyond the axis)
      __syncthreads();
      // consecutive threads on consecutive columns of a row (contiguous in memory when ts == inner)
      for (int x = threadIdx.x; x < nx * ts; x += kThreads) {
        const int r = x / ts, sl = x - r * ts;
        const int i = i0 + r;
        const size_t e = base + (size_t)i * inner + sl;
        pa[sl * kCorrA + r] = p[e];
        qa[sl * kCorrA + r] = q[e];
      }
      for (int x = threadIdx.x; x < nw * ts; x += kThreads) {
        const int r = x / ts, sl = x - r * ts;
        const int i = i0 + l0 + r;
        const size_t e = base + (size_t)i * inner + sl;
        pw[sl * kCorrW + r] = i < Mk ? p[e] : 0.f;
        qw[sl * kCorrW + r] = i < Mk ? q[e] : 0.f;
      }
      __syncthreads();
      for (int sl = 0; wave_live && sl < ts; ++sl) {
        const float* pas = pa + sl * kCorrA;
        const float* qas = qa + sl * kCorrA;
        const float* pws = pw + sl * kCorrW + threadIdx.x;
        const float* qws = qw + sl * kCorrW + threadIdx.x;
#pragma unroll 8
        for (int x = 0; x < nx; ++x) {
          a1 = fmaf(pas[x], qws[x], a1);
          a2 = fmaf(pws[x], qas[x], a2);
        }
      }
    }
  }
  if (l < Mk) part[(chunk * B + b) * Mk + l] = l == 0 ? a1 : a1 + a2;
}

// g[b, l] (row stride gstride) = sum of the chunks' partials, ascending
__global__ __launch_bounds__(kThreads) void k_grid_corr_reduce(const float* __restrict__ part, int chunks, int64_t B,
                                                                int Mk, int64_t gstride, float* __restrict__ g) {
  const size_t total = (size_t)B * Mk;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    float acc = part[e];
    for (int ch = 1; ch < chunks; ++ch) acc += part[(size_t)ch * total + e];
    g[(e / Mk) * gstride + e % Mk] = acc;
  }
}

// the chunking of one axis: enough workgroups to fill the device, at most 65535 chunks (a function of the shape alone)
struct CorrSplit {
  int lag_blocks, stiles, chunks;
  int64_t units, per_chunk;
};
static CorrSplit corr_split(int64_t B, int64_t outer, int64_t Mk, int64_t inner) {
  CorrSplit c;
  c.lag_blocks = (int)((Mk + kThreads - 1) / kThreads);
  c.stiles = (int)((inner + kCorrS - 1) / kCorrS);
  c.units = outer * c.stiles;
  int64_t want = (1024 + B * c.lag_blocks - 1) / (B * c.lag_blocks);
  want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, c.units), 65535));
  c.per_chunk = (c.units + want - 1) / want;
  c.chunks = (int)((c.units + c.per_chunk - 1) / c.per_chunk);
  return c;
}

static int grid_axis_corr(const float* p, const float* q, int64_t B, int64_t outer, int64_t Mk, int64_t inner,
                          float* part, float* g, int64_t gstride, hipStream_t st) {
  const CorrSplit c = corr_split(B, outer, Mk, inner);
  if (B > 65535) return LO_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_grid_axis_corr, dim3((unsigned)c.lag_blocks, (unsigned)c.chunks, (unsigned)B), dim3(kThreads), 0,
                     st, p, q, (int)Mk, outer, inner, c.stiles, c.units, c.per_chunk, part);
  const size_t total = (size_t)B * Mk;
  hipLaunchKernelGGL(k_grid_corr_reduce, dim3((unsigned)std::min<size_t>((total + kThreads - 1) / kThreads, 1024)),
                     dim3(kThreads), 0, st, part, c.chunks, B, (int)Mk, gstride, g);
  return LO_OK;
}

// workspace of the column gradients: nvec grid vectors [B, M, S] (2 for D = 2, 4 for D = 3) and the partials of the
// axis that needs most; the one layout, measured and carved by the same code
struct BilBufs {
  float* vec[4];
  float* part;
};
static void bil_layout(Arena& ar, const int64_t* m, int ndim, int64_t B, int64_t M, int64_t S, BilBufs* b) {
  for (int i = 0; i < (ndim == 2 ? 2 : 4); ++i) b->vec[i] = ar.take<float>((size_t)B * M * S);
  size_t part = 0;
  int64_t outer = 1;
  for (int k = 0; k < ndim; ++k) {
    const CorrSplit c = corr_split(B, outer, m[k], M / (outer * m[k]) * S);
    part = std::max(part, (size_t)c.chunks * B * m[k]);
    outer *= m[k];
  }
  b->part = ar.take<float>(part);
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_toeplitz_kron_workspace_bytes(const int64_t* m, int ndim, int64_t B, int64_t c) {
  int64_t M = 0;
  if (!m || B < 1 || c < 1 || !grid_shape_ok(m, ndim, &M)) return 0;
  return toeplitz_kron_ws_bytes(B, M, c);
}

int lo_toeplitz_kron_mv_f32(const float* t, const int64_t* m, int ndim, int64_t B, const float* u, int64_t c, float* y,
                            void* ws, size_t ws_bytes, void* stream) {
  if (!t || !m || !u || !y || !ws || B < 1 || c < 1 || u == y) return LO_ERR_BADARG;
  if (ndim != 2 && ndim != 3) return LO_ERR_UNSUPPORTED;
  for (int k = 0; k < ndim; ++k)
    if (m[k] < 1) return LO_ERR_BADARG;
  int64_t M = 0;
  if (!grid_shape_ok(m, ndim, &M)) return LO_ERR_UNSUPPORTED;
  if (c > INT_MAX / 64 || (size_t)B * M * c > (size_t)1 << 40) return LO_ERR_UNSUPPORTED;
  if (ws_bytes < toeplitz_kron_ws_bytes(B, M, c) - 256) return LO_ERR_WORKSPACE;
  // u -> ws -> y (D = 2), u -> y -> ws -> y (D = 3): the last pass writes y
  float* out = nullptr;
  float* w = (float*)ws;
  const int rc = ndim == 2 ? toeplitz_kron_passes(t, m, ndim, B, c, u, y, w, &out, nullptr, (hipStream_t)stream)
                           : toeplitz_kron_passes(t, m, ndim, B, c, u, w, y, &out, nullptr, (hipStream_t)stream);
  return rc;
}

size_t lo_toeplitz_kron_bilinear_workspace_bytes(const int64_t* m, int ndim, int64_t B, int64_t S) {
  int64_t M = 0;
  if (!m || B < 1 || S < 1 || !grid_shape_ok(m, ndim, &M)) return 0;
  BilBufs b;
  return measured(256, [&](Arena& ar) { bil_layout(ar, m, ndim, B, M, S, &b); });
}

int lo_toeplitz_kron_bilinear_f32(const float* t, const int64_t* m, int ndim, int64_t B, const float* u, const float* v,
                                  int64_t S, float* g, void* ws, size_t ws_bytes, void* stream) {
  if (!t || !m || !u || !v || !g || !ws || B < 1 || S < 1) return LO_ERR_BADARG;
  if (ndim != 2 && ndim != 3) return LO_ERR_UNSUPPORTED;
  for (int k = 0; k < ndim; ++k)
    if (m[k] < 1) return LO_ERR_BADARG;
  int64_t M = 0;
  if (!grid_shape_ok(m, ndim, &M)) return LO_ERR_UNSUPPORTED;
  if (S > INT_MAX / 64 || B > 65535 || (size_t)B * M * S > (size_t)1 << 40) return LO_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes);
  BilBufs w;
  bil_layout(ar, m, ndim, B, M, S, &w);
  if (!ar.ok) return LO_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const GridDiag none{nullptr, LO_DIAG_NONE, nullptr};
  int64_t sumM = 0;
  for (int k = 0; k < ndim; ++k) sumM += m[k];
  // axis k as [B * outer_k, m_k, inner_k]
  int64_t outer[3], inner[3], toff[3];
  for (int k = 0, o = 1, off = 0; k < ndim; ++k) {
    outer[k] = o;
    inner[k] = M / (o * m[k]) * S;
    toff[k] = off;
    o *= (int)m[k];
    off += (int)m[k];
  }
  auto pass = [&](int k, const float* src, float* dst) {
    return grid_axis(t + toff[k], sumM, B, outer[k], m[k], inner[k], src, dst, none, nullptr, st);
  };
  auto corr = [&](int k, const float* p, const float* q) {
    return grid_axis_corr(p, q, B, outer[k], m[k], inner[k], w.part, g + toff[k], sumM, st);
  };
  LO_PROF_BEGIN("toeplitz_kron_bilinear", st);
  int rc;
  if (ndim == 2) {
    // 2 passes: g_1 = corr_1(u, T_2 v), g_2 = corr_2(u, T_1 v)
    rc = pass(1, v, w.vec[0]);
    if (!rc) rc = corr(0, u, w.vec[0]);
    if (!rc) rc = pass(0, v, w.vec[1]);
    if (!rc) rc = corr(1, u, w.vec[1]);
  } else {
    // 4 passes instead of 6: with a = T_3 v and b = T_1 u (every factor is symmetric and acts on its own axis),
    //   g_2 = corr_2(b, a),  g_1 = corr_1(u, T_2 a),  g_3 = corr_3(b, T_2 v).
    // (3 passes cannot do: each pair of axes must sit on opposite sides of one correlation -- an odd cycle.)
    float *a = w.vec[0], *b = w.vec[1], *c = w.vec[2], *e = w.vec[3];
    rc = pass(2, v, a);
    if (!rc) rc = pass(0, u, b);
    if (!rc) rc = corr(1, b, a);
    if (!rc) rc = pass(1, a, c);
    if (!rc) rc = corr(0, u, c);
    if (!rc) rc = pass(1, v, e);
    if (!rc) rc = corr(2, b, e);
  }
  LO_PROF_END(st);
  if (rc) return rc;
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // extern "C"
