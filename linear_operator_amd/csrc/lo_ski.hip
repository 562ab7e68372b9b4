// lo_ski.hip -- structured kernel interpolation (KISS-GP / SKI): K ~= W_l T W_r^T with T a symmetric Toeplitz matrix on a
// regular grid of M points and W a sparse interpolation matrix of J nonzeros per row.
//   InterpolatedLinearOperator._matmul     (interpolated_linear_operator.py:192-219)
//   ToeplitzLinearOperator._matmul         (toeplitz_linear_operator.py:42-53, utils/toeplitz.py sym_toeplitz_matmul)
//   sym_toeplitz_derivative_quadratic_form (utils/toeplitz.py), the interpolation-value gradient
//                                          (interpolated_linear_operator.py:293-323)
//
// Kernels
//   k_interp        y = W u (+ d o v): one thread per output element, J gathers from the grid-sized u (L2 resident).
//   k_csr_*         grid-major (CSR) copy of W, built once per plan: integer counting sort (count, scan, fill) and a
//                   rank sort of every grid point's entries by entry id, so the entries of a grid point are in
//                   ascending (n, j) order whatever order the fill's integer atomics ran in.
//   k_interp_t_*    W^T v as a segmented gather-sum over that copy (a wave per grid point and column below 8 columns,
//                   a lane per output element above): deterministic (no float atomics).
//   k_tz_mv         T u, direct O(M^2 c) product from LDS: a workgroup owns 256 rows and a slice of the k range; the
//                   lags of a (256 row x 256 k) tile are a window of 511 entries of the column staged in LDS next to
//                   the u tile, so no M x M matrix exists anywhere.  Up to 32 columns per launch; split-k partials are
//                   summed in fixed order by k_tz_reduce (which also carries the + d o v epilogue of the Toeplitz kind).
//   k_tz_bil        the lag correlation g_k = sum_s sum_i (u_{s,i} v_{s,i+k} + u_{s,i+k} v_{s,i}), g_0 = sum u o v: a
//                   thread per lag, i tiles staged in LDS with the shifted windows, split-i partials reduced in order.
//   k_interp_vgrad  dvals[n, j] = sum_s lv[n, s] R[idx[n, j], s].
// Index entries outside [0, M) contribute nothing: no kernel reads outside the arrays it was given.
#include <algorithm>
#include <climits>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

constexpr int kTzRows = 256;  // output rows of a k_tz_mv workgroup (one per thread)
constexpr int kTzK = 256;     // k tile
constexpr int kTzMaxCols = 32;

// ---- interpolation, gather side -------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_interp(const int64_t* __restrict__ idx, const float* __restrict__ vals,
                                                      int64_t B, int64_t N, int J, int64_t M, const float* __restrict__ u,
                                                      int c, const float* __restrict__ dd, int dd_mode,
                                                      const float* __restrict__ v, float* __restrict__ y,
                                                      const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t total = (size_t)B * N * c;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t row = e / c;  // b * N + n
    const int col = (int)(e % c);
    const size_t b = row / N;
    const int64_t* ir = idx + row * J;
    const float* wr = vals + row * J;
    const float* ub = u + b * M * c + col;
    float acc = 0.f;
    for (int j = 0; j < J; ++j) {
      const int64_t m = ir[j];
      const float g = (m >= 0 && m < M) ? ub[m * c] : 0.f;
      acc = fmaf(g, wr[j], acc);
    }
    if (dd_mode == LO_DIAG_FULL) acc = fmaf(dd[row], v[e], acc);
    else if (dd_mode == LO_DIAG_CONST) acc = fmaf(dd[b], v[e], acc);
    y[e] = acc;
  }
}

static unsigned grid_for(size_t total) {
  const size_t g = (total + kThreads - 1) / kThreads;
  return (unsigned)std::max<size_t>(1, std::min<size_t>(g, 8192));
}

bool interp_shape_ok(int64_t B, int64_t N, int64_t J, int64_t M) {
  return B >= 1 && N >= 1 && J >= 1 && M >= 1 && N * J <= INT_MAX - 1 && M <= INT_MAX - 2;
}

int interp_gather(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* u,
                  int64_t c, const float* dd, int dd_mode, const float* v, float* y, const int* stop, hipStream_t st) {
  if (!interp_shape_ok(B, N, J, M) || c < 1 || c > INT_MAX) return LO_ERR_BADARG;
  const size_t total = (size_t)B * N * c;
  LO_PROF_BEGIN("ski_interp", st);
  hipLaunchKernelGGL(k_interp, dim3(grid_for(total)), dim3(kThreads), 0, st, idx, vals, B, N, (int)J, M, u, (int)c, dd,
                     dd_mode, v, y, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// ---- grid-major copy of W (built once per plan) ----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_csr_count(const int64_t* __restrict__ idx, int64_t B, int NJ, int64_t M,
                                                         int* __restrict__ cnt) {
  const size_t total = (size_t)B * NJ;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const int64_t m = idx[e];
    if (m >= 0 && m < M) atomicAdd(&cnt[(e / NJ) * (M + 1) + m], 1);  // (integer counts: order-free)
  }
}

// exclusive scan of the M + 1 counts of one member in place (ptr[M] = entries of the member); cur = a copy of ptr
__global__ __launch_bounds__(kThreads) void k_csr_scan(int* __restrict__ ptr, int* __restrict__ cur, int64_t M) {
  __shared__ int tot[kThreads];
  const int64_t L = M + 1;
  int* p = ptr + (size_t)blockIdx.x * L;
  int* q = cur + (size_t)blockIdx.x * L;
  const int64_t chunk = (L + kThreads - 1) / kThreads;
  const int64_t a = std::min<int64_t>(L, threadIdx.x * chunk), z = std::min<int64_t>(L, a + chunk);
  int s = 0;
  for (int64_t i = a; i < z; ++i) s += p[i];
  tot[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < kThreads; ++t) {
      const int x = tot[t];
      tot[t] = run;
      run += x;
    }
  }
  __syncthreads();
  int run = tot[threadIdx.x];
  for (int64_t i = a; i < z; ++i) {
    const int x = p[i];
    p[i] = run;
    q[i] = run;
    run += x;
  }
}

__global__ __launch_bounds__(kThreads) void k_csr_fill(const int64_t* __restrict__ idx, int64_t B, int NJ, int64_t M,
                                                        int* __restrict__ cur, int* __restrict__ ids) {
  const size_t total = (size_t)B * NJ;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const int64_t m = idx[e];
    if (m >= 0 && m < M) {
      const size_t b = e / NJ;
      const int pos = atomicAdd(&cur[b * (M + 1) + m], 1);
      ids[b * NJ + pos] = (int)(e - b * NJ);
    }
  }
}

// the entries of every grid point in ascending entry order, one wave per point: rank of an id = number of smaller ids
// in the segment (ids are unique)
__global__ __launch_bounds__(kThreads) void k_csr_sort(const int* __restrict__ ptr, int64_t B, int NJ, int64_t M,
                                                        const int* __restrict__ in, int* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const size_t total = (size_t)B * M;
  for (size_t bm = (size_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6); bm < total;
       bm += (size_t)gridDim.x * (kThreads / 64)) {
    const size_t b = bm / M, m = bm % M;
    const int beg = ptr[b * (M + 1) + m], end = ptr[b * (M + 1) + m + 1];
    const int* seg = in + b * NJ + beg;
    int* dst = out + b * NJ + beg;
    const int n = end - beg;
    for (int i = lane; i < n; i += 64) {
      const int id = seg[i];
      int r = 0;
      for (int k = 0; k < n; ++k) r += seg[k] < id;
      dst[r] = id;
    }
  }
}

void csr_layout(Arena& ar, int64_t B, int64_t N, int64_t J, int64_t M, CsrBufs* b) {
  b->ptr = ar.take<int>((size_t)B * (M + 1));
  b->cur = ar.take<int>((size_t)B * (M + 1));
  b->tmp = ar.take<int>((size_t)B * N * J);
  b->ids = ar.take<int>((size_t)B * N * J);
}

size_t csr_bytes(int64_t B, int64_t N, int64_t J, int64_t M) {
  CsrBufs b;
  return measured(kPlanTail, [&](Arena& ar) { csr_layout(ar, B, N, J, M, &b); });
}

int csr_build(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, Arena* ar, CsrBufs* b, hipStream_t st) {
  if (!interp_shape_ok(B, N, J, M)) return LO_ERR_BADARG;
  csr_layout(*ar, B, N, J, M, b);
  if (ar->measuring()) return LO_OK;
  if (!ar->ok) return LO_ERR_WORKSPACE;
  const int NJ = (int)(N * J);
  LO_HIP_CHECK(hipMemsetAsync(b->ptr, 0, sizeof(int) * (size_t)B * (M + 1), st));
  const size_t total = (size_t)B * NJ;
  LO_PROF_BEGIN("ski_csr_build", st);
  hipLaunchKernelGGL(k_csr_count, dim3(grid_for(total)), dim3(kThreads), 0, st, idx, B, NJ, M, b->ptr);
  hipLaunchKernelGGL(k_csr_scan, dim3((unsigned)B), dim3(kThreads), 0, st, b->ptr, b->cur, M);
  hipLaunchKernelGGL(k_csr_fill, dim3(grid_for(total)), dim3(kThreads), 0, st, idx, B, NJ, M, b->cur, b->tmp);
  const unsigned sgrid = (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)B * M + 3) / 4, 32768));
  hipLaunchKernelGGL(k_csr_sort, dim3(sgrid), dim3(kThreads), 0, st, b->ptr, B, NJ, M, b->tmp, b->ids);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

CsrBufs csr_view(const void* plan, int64_t B, int64_t N, int64_t J, int64_t M) {
  Arena ar(const_cast<void*>(plan), SIZE_MAX);
  CsrBufs b;
  csr_layout(ar, B, N, J, M, &b);
  return b;
}

// ---- interpolation, scatter side: out[b, m, col] = sum over the entries (n, j) at grid point m of vals * v[n, col] --
// one wave per (member, grid point, column): the lanes stride the point's entries (their loads in flight together
// instead of one dependent chain per thread), then the fixed-order wave butterfly -- bitwise the same every run
// few columns: one wave per (member, grid point, column)
__global__ __launch_bounds__(kThreads) void k_interp_t_wave(const int* __restrict__ ptr, const int* __restrict__ ids,
                                                        const float* __restrict__ vals, int64_t B, int64_t N, int J,
                                                        int64_t M, const float* __restrict__ v, int vdiv, int c,
                                                        float* __restrict__ out, const int* __restrict__ stop) {
  if (stop && *stop) return;
  constexpr int kWaves = kThreads / 64;
  const int lane = threadIdx.x & 63;
  const size_t total = (size_t)B * M * c;
  const int NJ = (int)(N * J);
  for (size_t e = (size_t)blockIdx.x * kWaves + (threadIdx.x >> 6); e < total; e += (size_t)gridDim.x * kWaves) {
    const size_t bm = e / c;
    const int col = (int)(e % c);
    const size_t b = bm / M;
    const size_t m = bm % M;
    const int* pb = ptr + b * (M + 1);
    const int beg = pb[m], end = pb[m + 1];
    const int* ib = ids + b * NJ;
    const float* wb = vals + b * NJ;
    const float* vb = v + (vdiv > 1 ? b / vdiv : b) * N * c + col;
    float acc = 0.f;
    for (int k = beg + lane; k < end; k += 64) {
      const int id = ib[k];
      acc = fmaf(wb[id], vb[(size_t)(id / J) * c], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[e] = acc;
  }
}

// many columns: one thread per output element, the columns of a grid point in consecutive lanes (shared index loads)
__global__ __launch_bounds__(kThreads) void k_interp_t_lane(const int* __restrict__ ptr, const int* __restrict__ ids,
                                                             const float* __restrict__ vals, int64_t B, int64_t N, int J,
                                                             int64_t M, const float* __restrict__ v, int vdiv, int c,
                                                             float* __restrict__ out, const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t total = (size_t)B * M * c;
  const int NJ = (int)(N * J);
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t bm = e / c;
    const int col = (int)(e % c);
    const size_t b = bm / M;
    const size_t m = bm % M;
    const int* pb = ptr + b * (M + 1);
    const int beg = pb[m], end = pb[m + 1];
    const int* ib = ids + b * NJ;
    const float* wb = vals + b * NJ;
    const float* vb = v + (vdiv > 1 ? b / vdiv : b) * N * c + col;
    float acc = 0.f;
    for (int k = beg; k < end; ++k) {
      const int id = ib[k];
      acc = fmaf(wb[id], vb[(size_t)(id / J) * c], acc);
    }
    out[e] = acc;
  }
}

// vdiv: grid members that read one member of v (member b of W reads v[b / vdiv]): 1 for the SKI kinds, the P terms of
// the additive kind (lo_ski_sum.hip), whose v [B / P, N, c] is never copied P times
int interp_scatter_bcast(const int* ptr, const int* ids, const float* vals, int64_t B, int vdiv, int64_t N, int64_t J,
                         int64_t M, const float* v, int64_t c, float* out, const int* stop, hipStream_t st) {
  if (!interp_shape_ok(B, N, J, M) || c < 1 || c > INT_MAX || vdiv < 1) return LO_ERR_BADARG;
  const size_t total = (size_t)B * M * c;
  LO_PROF_BEGIN("ski_interp_t", st);
  if (c < 8) {  // (the mode is a function of the shape only: the same inputs give the same bits)
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((total + 3) / 4, 32768));
    hipLaunchKernelGGL(k_interp_t_wave, dim3(grid), dim3(kThreads), 0, st, ptr, ids, vals, B, N, (int)J, M, v, vdiv,
                       (int)c, out, stop);
  } else {
    hipLaunchKernelGGL(k_interp_t_lane, dim3(grid_for(total)), dim3(kThreads), 0, st, ptr, ids, vals, B, N, (int)J, M, v,
                       vdiv, (int)c, out, stop);
  }
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int interp_scatter(const int* ptr, const int* ids, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M,
                   const float* v, int64_t c, float* out, const int* stop, hipStream_t st) {
  return interp_scatter_bcast(ptr, ids, vals, B, 1, N, J, M, v, c, out, stop, st);
}

// ---- Toeplitz product --------------------------------------------------------------------------------------------------
struct TzSplit {
  int RB;  // row blocks of kTzRows
  int KS;  // k slices
  int kchunk;
};

static TzSplit tz_split(int64_t B, int64_t M) {
  TzSplit s;
  s.RB = (int)((M + kTzRows - 1) / kTzRows);
  const int maxks = (int)((M + kTzK - 1) / kTzK);
  int ks = (int)((512 + B * s.RB - 1) / (B * s.RB));
  s.KS = std::max(1, std::min(ks, maxks));
  s.kchunk = (int)(((M + s.KS - 1) / s.KS + kTzK - 1) / kTzK * kTzK);
  s.KS = (int)((M + s.kchunk - 1) / s.kchunk);
  return s;
}

// part[(ks * B + b) * M + i][c] (columns col0 .. col0 + cc) = sum_{k in slice ks} t[|i - k|] u[b, k, col]
template <int CB>
__global__ __launch_bounds__(kThreads) void k_tz_mv(const float* __restrict__ t, int M, const float* __restrict__ u,
                                                     int c, int col0, int cc, int kchunk, float* __restrict__ part,
                                                     const int* __restrict__ stop) {
  if (stop && *stop) return;
  __shared__ float us[kTzK * CB];
  __shared__ float win[kTzRows + kTzK];
  const int i0 = blockIdx.x * kTzRows;
  const int ks = blockIdx.y;
  const size_t b = blockIdx.z;
  const size_t B = gridDim.z;
  const int kb = ks * kchunk, ke = min(M, kb + kchunk);
  const float* tb = t + b * M;
  const float* ub = u + b * (size_t)M * c + col0;
  const int i = i0 + threadIdx.x;
  float acc[CB];
#pragma unroll
  for (int q = 0; q < CB; ++q) acc[q] = 0.f;
  for (int k0 = kb; k0 < ke; k0 += kTzK) {
    __syncthreads();
    for (int e = threadIdx.x; e < kTzK * CB; e += kThreads) {
      const int kk = e / CB, q = e % CB;
      const int k = k0 + kk;
      us[e] = (k < ke && q < cc) ? ub[(size_t)k * c + q] : 0.f;
    }
    // lags i - k for i in [i0, i0 + 256), k in [k0, k0 + 256): d = dmin + x, x in [0, 511)
    const int dmin = i0 - k0 - (kTzK - 1);
    for (int x = threadIdx.x; x < kTzRows + kTzK - 1; x += kThreads) {
      const int dd = dmin + x;
      const int ad = dd < 0 ? -dd : dd;
      win[x] = ad < M ? tb[ad] : 0.f;
    }
    __syncthreads();
    const float* w = win + threadIdx.x + (kTzK - 1);  // w[-kk] = t[|i - (k0 + kk)|]
#pragma unroll 4
    for (int kk = 0; kk < kTzK; ++kk) {
      const float a = w[-kk];
#pragma unroll
      for (int q = 0; q < CB; ++q) acc[q] = fmaf(a, us[kk * CB + q], acc[q]);
    }
  }
  if (i < M) {
    float* pp = part + ((size_t)ks * B + b) * (size_t)M * c + (size_t)i * c + col0;
#pragma unroll
    for (int q = 0; q < CB; ++q)
      if (q < cc) pp[q] = acc[q];
  }
}

// y[e] = sum_s part[s][e] (fixed order) (+ d o v)
__global__ __launch_bounds__(kThreads) void k_tz_reduce(const float* __restrict__ part, int KS, int64_t B, int64_t M,
                                                         int c, const float* __restrict__ dd, int dd_mode,
                                                         const float* __restrict__ v, float* __restrict__ y,
                                                         const int* __restrict__ stop) {
  if (stop && *stop) return;
  const size_t total = (size_t)B * M * c;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    float acc = part[e];
    for (int s = 1; s < KS; ++s) acc += part[(size_t)s * total + e];
    if (dd_mode == LO_DIAG_FULL) acc = fmaf(dd[e / c], v[e], acc);
    else if (dd_mode == LO_DIAG_CONST) acc = fmaf(dd[e / ((size_t)M * c)], v[e], acc);
    y[e] = acc;
  }
}

size_t toeplitz_part_floats(int64_t B, int64_t M, int64_t c) { return (size_t)tz_split(B, M).KS * B * M * c; }

size_t toeplitz_part_bytes(int64_t B, int64_t M, int64_t c) {
  return align_up(toeplitz_part_floats(B, M, c) * sizeof(float), 256) + 256;
}

int toeplitz_mv(const float* t, int64_t B, int64_t M, const float* u, int64_t c, const float* dd, int dd_mode,
                const float* v, float* y, float* part, const int* stop, hipStream_t st) {
  if (B < 1 || M < 1 || c < 1 || !t || !u || !y || !part) return LO_ERR_BADARG;
  if (M > LO_TOEPLITZ_MAX_M || c > INT_MAX / LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  const TzSplit s = tz_split(B, M);
  dim3 grid((unsigned)s.RB, (unsigned)s.KS, (unsigned)B);
  LO_PROF_BEGIN("ski_toeplitz_mv", st);
  for (int64_t col0 = 0; col0 < c; col0 += kTzMaxCols) {
    const int cc = (int)std::min<int64_t>(kTzMaxCols, c - col0);
#define LO_TZ_LAUNCH(CBV) \
  hipLaunchKernelGGL((k_tz_mv<CBV>), grid, dim3(kThreads), 0, st, t, (int)M, u, (int)c, (int)col0, cc, s.kchunk, part, stop)
    if (cc <= 1) LO_TZ_LAUNCH(1);
    else if (cc <= 2) LO_TZ_LAUNCH(2);
    else if (cc <= 4) LO_TZ_LAUNCH(4);
    else if (cc <= 8) LO_TZ_LAUNCH(8);
    else if (cc <= 16) LO_TZ_LAUNCH(16);
    else if (cc <= 24) LO_TZ_LAUNCH(24);
    else LO_TZ_LAUNCH(32);
#undef LO_TZ_LAUNCH
  }
  hipLaunchKernelGGL(k_tz_reduce, dim3(grid_for((size_t)B * M * c)), dim3(kThreads), 0, st, part, s.KS, B, M, (int)c,
                     dd, dd_mode, v, y, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// ---- lag correlation (backward of the Toeplitz column) -----------------------------------------------------------------
constexpr int kBilI = 256;

__global__ __launch_bounds__(kThreads) void k_tz_bil(const float* __restrict__ u, const float* __restrict__ v, int M,
                                                      int S, int ichunk, float* __restrict__ part) {
  __shared__ float ua[kBilI], va[kBilI], uw[kBilI + kThreads], vw[kBilI + kThreads];
  const int k0 = blockIdx.x * kThreads;
  const int ks = blockIdx.y;
  const size_t b = blockIdx.z, B = gridDim.z;
  const int k = k0 + threadIdx.x;
  const int ib = ks * ichunk, ie = min(M, ib + ichunk);
  const float* ub = u + b * (size_t)M * S;
  const float* vb = v + b * (size_t)M * S;
  float a1 = 0.f, a2 = 0.f;
  for (int i0 = ib; i0 < ie; i0 += kBilI) {
    for (int s = 0; s < S; ++s) {
      __syncthreads();
      for (int x = threadIdx.x; x < kBilI; x += kThreads) {
        const int i = i0 + x;
        ua[x] = i < ie ? ub[(size_t)i * S + s] : 0.f;
        va[x] = i < ie ? vb[(size_t)i * S + s] : 0.f;
      }
      for (int x = threadIdx.x; x < kBilI + kThreads; x += kThreads) {
        const int i = i0 + k0 + x;
        uw[x] = i < M ? ub[(size_t)i * S + s] : 0.f;
        vw[x] = i < M ? vb[(size_t)i * S + s] : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int x = 0; x < kBilI; ++x) {
        a1 = fmaf(ua[x], vw[x + threadIdx.x], a1);
        a2 = fmaf(uw[x + threadIdx.x], va[x], a2);
      }
    }
  }
  if (k < M) part[((size_t)ks * B + b) * M + k] = k == 0 ? a1 : a1 + a2;
}

static void bil_split(int64_t B, int64_t M, int* LB, int* KI, int* ichunk) {
  *LB = (int)((M + kThreads - 1) / kThreads);
  const int maxki = (int)((M + kBilI - 1) / kBilI);
  int ki = (int)((512 + B * *LB - 1) / (B * *LB));
  ki = std::max(1, std::min(ki, maxki));
  *ichunk = (int)(((M + ki - 1) / ki + kBilI - 1) / kBilI * kBilI);
  *KI = (int)((M + *ichunk - 1) / *ichunk);
}

size_t toeplitz_bil_bytes(int64_t B, int64_t M) {
  int LB, KI, ic;
  bil_split(B, M, &LB, &KI, &ic);
  return align_up((size_t)KI * B * M * sizeof(float), 256) + 256;
}

// ---- interpolation-value gradient --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_interp_vgrad(const int64_t* __restrict__ idx, int64_t B, int64_t N, int J,
                                                            int64_t M, const float* __restrict__ lv,
                                                            const float* __restrict__ R, int S, float* __restrict__ g) {
  const size_t total = (size_t)B * N * J;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t row = e / J;
    const size_t b = row / N;
    const int64_t m = idx[e];
    float acc = 0.f;
    if (m >= 0 && m < M) {
      const float* l = lv + row * S;
      const float* r = R + (b * M + m) * S;
      for (int s = 0; s < S; ++s) acc = fmaf(l[s], r[s], acc);
    }
    g[e] = acc;
  }
}

// ---- pieces of the matvec plan (lo_matvec.hip) --------------------------------------------------------------------------
int ski_interp_plan(MatvecPlan* pl, int64_t M, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  SkiPlan& k = pl->ski;
  k.w = *op.interp;
  k.u = ar->take<float>((size_t)op.B * M * pl->c);
  k.t = ar->take<float>((size_t)op.B * M * pl->c);
  if (!ar->ok) return LO_ERR_WORKSPACE;
  if (k.w.right_plan) {  // the caller keeps the grid-major copy of W_r across calls (lo_interp_plan_build)
    k.csr = csr_view(k.w.right_plan, op.B, op.N, op.n2, M);
    return LO_OK;
  }
  return csr_build(k.w.right_idx, op.B, op.N, op.n2, M, ar, &k.csr, st);
}

int toeplitz_desc_check(const lo_op_desc* op) { return (!op->A0 || op->R != op->N) ? LO_ERR_BADARG : LO_OK; }

int ski_desc_check(const lo_op_desc* op) {
  return (!op->A0 || op->R < 1 || op->n2 < 1 || !interp_ptrs_ok(op->interp)) ? LO_ERR_BADARG : LO_OK;
}

int ski_plan(MatvecPlan* pl, Arena* ar, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const int64_t M = op.R;
  const bool tz = op.kind == LO_OP_TOEPLITZ_DIAG;
  const int bad = tz ? toeplitz_desc_check(&op) : ski_desc_check(&op);
  // The order of the refusals, kept as it always was: (1) no column: BADARG; (2) M beyond the bound of the Toeplitz
  // product: UNSUPPORTED (the plan's own condition -- the pivoted Cholesky reads single entries and has no such bound);
  // (3) whatever else the shared check found: BADARG; (4) the products' own shape limits: BADARG
  if (op.A0 && M > LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  if (bad) return bad;
  if (tz ? M < 1 : !interp_shape_ok(op.B, op.N, op.n2, M)) return LO_ERR_BADARG;  // (the 32-bit limits of the products)
  if (!tz) {
    const int rc = ski_interp_plan(pl, M, ar, st);
    if (rc) return rc;
  }
  pl->ski.tz_part = ar->take<float>(toeplitz_part_floats(op.B, M, pl->c));
  return LO_OK;
}

int ski_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  const SkiPlan& k = pl->ski;
  const int64_t M = op.R;
  if (op.kind == LO_OP_TOEPLITZ_DIAG)
    return toeplitz_mv(op.A0, op.B, M, v, pl->c, op.d, op.diag_mode, v, y, k.tz_part, stop, st);
  int rc = interp_scatter(k.csr.ptr, k.csr.ids, k.w.right_vals, op.B, op.N, op.n2, M, v, pl->c, k.u, stop, st);
  if (!rc) rc = toeplitz_mv(op.A0, op.B, M, k.u, pl->c, nullptr, LO_DIAG_NONE, nullptr, k.t, k.tz_part, stop, st);
  if (!rc) rc = interp_gather(k.w.left_idx, k.w.left_vals, op.B, op.N, op.n2, M, k.t, pl->c, op.d, op.diag_mode, v, y,
                              stop, st);
  return rc;
}

}  // namespace lo

using namespace lo;

extern "C" {

int lo_interp_f32(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* u,
                  int64_t c, float* y, void* stream) {
  if (!idx || !vals || !u || !y) return LO_ERR_BADARG;
  return interp_gather(idx, vals, B, N, J, M, u, c, nullptr, LO_DIAG_NONE, nullptr, y, nullptr, (hipStream_t)stream);
}

size_t lo_interp_t_workspace_bytes(int64_t B, int64_t N, int64_t J, int64_t M) {
  if (!interp_shape_ok(B, N, J, M)) return 0;
  return csr_bytes(B, N, J, M);
}

int lo_interp_t_f32(const int64_t* idx, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M, const float* v,
                    int64_t c, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!idx || !vals || !v || !out || !ws) return LO_ERR_BADARG;
  if (!interp_shape_ok(B, N, J, M)) return LO_ERR_BADARG;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes);
  CsrBufs b;
  const int rc = csr_build(idx, B, N, J, M, &ar, &b, st);
  if (rc) return rc;
  return interp_scatter(b.ptr, b.ids, vals, B, N, J, M, v, c, out, nullptr, st);
}

size_t lo_interp_plan_bytes(int64_t B, int64_t N, int64_t J, int64_t M) {
  if (!interp_shape_ok(B, N, J, M)) return 0;
  return csr_bytes(B, N, J, M);
}

int lo_interp_plan_build(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, void* plan, size_t plan_bytes,
                         void* stream) {
  if (!idx || !plan || !interp_shape_ok(B, N, J, M)) return LO_ERR_BADARG;
  if (plan_bytes < csr_bytes(B, N, J, M)) return LO_ERR_WORKSPACE;
  Arena ar(plan, plan_bytes);
  CsrBufs b;
  return csr_build(idx, B, N, J, M, &ar, &b, (hipStream_t)stream);
}

int lo_interp_t_planned_f32(const void* plan, const float* vals, int64_t B, int64_t N, int64_t J, int64_t M,
                            const float* v, int64_t c, float* out, void* stream) {
  if (!plan || !vals || !v || !out || !interp_shape_ok(B, N, J, M)) return LO_ERR_BADARG;
  const CsrBufs b = csr_view(plan, B, N, J, M);
  return interp_scatter(b.ptr, b.ids, vals, B, N, J, M, v, c, out, nullptr, (hipStream_t)stream);
}

size_t lo_toeplitz_workspace_bytes(int64_t B, int64_t M, int64_t c) {
  if (B < 1 || M < 1 || c < 1) return 0;
  return std::max(toeplitz_part_bytes(B, M, c), toeplitz_bil_bytes(B, M));
}

int lo_toeplitz_mv_f32(const float* t, int64_t B, int64_t M, const float* u, int64_t c, float* y, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!t || !u || !y || !ws || B < 1 || M < 1 || c < 1) return LO_ERR_BADARG;
  if (M > LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  if (ws_bytes < toeplitz_part_bytes(B, M, c) - 256) return LO_ERR_WORKSPACE;
  return toeplitz_mv(t, B, M, u, c, nullptr, LO_DIAG_NONE, nullptr, y, (float*)ws, nullptr, (hipStream_t)stream);
}

int lo_toeplitz_bilinear_f32(const float* u, const float* v, int64_t B, int64_t M, int64_t S, float* g, void* ws,
                             size_t ws_bytes, void* stream) {
  if (!u || !v || !g || !ws || B < 1 || M < 1 || S < 1 || S > INT_MAX / LO_TOEPLITZ_MAX_M) return LO_ERR_BADARG;
  if (M > LO_TOEPLITZ_MAX_M) return LO_ERR_UNSUPPORTED;
  if (ws_bytes < toeplitz_bil_bytes(B, M) - 256) return LO_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int LB, KI, ichunk;
  bil_split(B, M, &LB, &KI, &ichunk);
  float* part = (float*)ws;
  LO_PROF_BEGIN("ski_toeplitz_bilinear", st);
  hipLaunchKernelGGL(k_tz_bil, dim3((unsigned)LB, (unsigned)KI, (unsigned)B), dim3(kThreads), 0, st, u, v, (int)M,
                     (int)S, ichunk, part);
  hipLaunchKernelGGL(k_tz_reduce, dim3(grid_for((size_t)B * M)), dim3(kThreads), 0, st, part, KI, B, M, 1, nullptr,
                     LO_DIAG_NONE, nullptr, g, nullptr);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int lo_interp_values_grad_f32(const int64_t* idx, int64_t B, int64_t N, int64_t J, int64_t M, const float* lv,
                              const float* R, int64_t S, float* g, void* stream) {
  if (!idx || !lv || !R || !g || S < 1 || S > INT_MAX) return LO_ERR_BADARG;
  if (!interp_shape_ok(B, N, J, M)) return LO_ERR_BADARG;
  hipStream_t st = (hipStream_t)stream;
  LO_PROF_BEGIN("ski_interp_vgrad", st);
  hipLaunchKernelGGL(k_interp_vgrad, dim3(grid_for((size_t)B * N * J)), dim3(kThreads), 0, st, idx, B, N, (int)J, M, lv,
                     R, (int)S, g);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // extern "C"
