// lo_chol.hip -- the exact small-N path (N <= 1024): batched lower Cholesky, triangular solves and the two-sided
// Cholesky solve, fp32, one workgroup per member (per member and column block for the solves).
// (reference: utils/cholesky.py:13-74 -> torch.linalg.cholesky_ex; triangular_linear_operator.py:72-191 ->
//  torch.linalg.solve_triangular; chol_linear_operator.py -> torch.cholesky_solve.)
//
// lo_cholesky_f32: blocked LEFT-looking factorisation, panels of 32 columns, in a padded workspace copy W [Np, Np],
// Np = N rounded up to 32 (blockdiag(A, I): chol(blockdiag(A, I)) = blockdiag(chol(A), I), so no loop has a ragged
// edge and every row of W is 16-byte aligned whatever N is).  Per panel:
//   1. the 32 finished rows L[col0 .. col0+31, 0 .. col0) go to LDS (the B operand every row tile shares);
//   2. every wave takes row tiles of 32: P = A[tile, panel] - L[tile, :col0] L[panel, :col0]^T on
//      v_mfma_f32_32x32x2_f32 (A operand straight from W, 64 contiguous bytes per lane and slab);
//   3. wave 0 factorises the 32 x 32 diagonal block in registers (lane = row, v_readlane broadcasts);
//   4. one thread per row below it substitutes against the block (broadcast LDS reads).
// Sums run in a fixed order, there is no atomic and no inter-workgroup communication: a member's factor does not depend
// on the batch it is in, and repeats bit for bit.  A pivot that is not > 0 records its 1-based order once; the arithmetic
// goes on (NaN / inf stay inside the member's own W and L).
//
// lo_tri_solve_f32 / lo_cholesky_solve_f32: blocked substitution, blocks of 32 rows, the N x CB tile of right-hand
// sides resident in LDS for the whole launch (both sweeps of the Cholesky solve included).  Per block: the update
// X[blk] -= M[blk, done] X[done] streams M in slabs of 128 through LDS, each of the 8 half-waves owning 16 k of the slab
// for all CB columns (so one column keeps the workgroup as busy as sixteen), a fixed-order sum of the 8 partials, then
// the 32 x 32 diagonal block is solved by a half-wave per column (lane = row, __shfl broadcasts).
#include "lo_internal.h"

namespace lo {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int CH_NB = 32;       // panel width / block rows
constexpr int CH_LDD = 33;      // row stride of the 32 x 32 diagonal block in LDS
constexpr int TS_KS = 128;      // k-slab of the substitution update
constexpr int kCholMaxN = 1024;

__device__ __forceinline__ int mfma_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ float lane_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// ---------------------------------------------------------------------------------------------------- factorisation
__global__ __launch_bounds__(kThreads) void k_chol_blocked(const float* __restrict__ A, float* __restrict__ W,
                                                           float* __restrict__ Lout, int* __restrict__ info,
                                                           double* __restrict__ logdet, double* __restrict__ dsum,
                                                           int N, int Np, int ldb) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  // (the fixed-size arrays are static: their addresses are immediates; behind the run-time base of the dynamic segment
  //  the unrolled substitution keeps 528 of them in SGPRs, and spills)
  __shared__ float Ds[CH_NB * CH_LDD];  // [32][33]    diagonal block
  __shared__ float dinv[CH_NB];         // [32]        1 / L_jj of the block
  float* Bs = sm;                       // [32][ldb]   finished rows of the panel, k-contiguous
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, h = lane >> 5;
  const float* Ab = A + (size_t)b * N * N;
  float* Wb = W + (size_t)b * Np * Np;
  // the pivots decide the log-determinant: sum_k L_rk^2 over the finished panels is kept per row in float64 and the
  // diagonal of each block starts from A_rr - that sum (the 32 x 32 block itself is float32)
  double* ds = dsum + (size_t)b * Np;
  for (int r = tid; r < Np; r += kThreads) ds[r] = 0.0;
  int first_bad = 0;   // wave 0 only (uniform)
  double ld = 0.0;     // wave 0 only: lane li sums log L_rr over its rows r = 32 p + li

  for (int col0 = 0; col0 < Np; col0 += CH_NB) {
    const int q4 = col0 >> 2;
    for (int idx = tid; idx < CH_NB * q4; idx += kThreads) {
      const int j = idx / q4, q = idx - j * q4;
      *reinterpret_cast<float4*>(Bs + j * ldb + 4 * q) =
          *reinterpret_cast<const float4*>(Wb + (size_t)(col0 + j) * Np + 4 * q);
    }
    __syncthreads();
    const int tiles = (Np - col0) / CH_NB;
    for (int t = wave; t < tiles; t += 4) {
      const int r0 = col0 + CH_NB * t;
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
      const float* ap = Wb + (size_t)(r0 + li) * Np + 16 * h;
      const float* bp = Bs + li * ldb + 16 * h;
      for (int k0 = 0; k0 < col0; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 a4 = *reinterpret_cast<const float4*>(ap + k0 + 4 * q);
          const float4 b4 = *reinterpret_cast<const float4*>(bp + k0 + 4 * q);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int lr = mfma_row(e, lane);
        const int row = r0 + lr, col = col0 + li;
        float a;
        if (row < N && col < N) a = (col <= row) ? Ab[(size_t)row * N + col] : 0.f;  // the lower triangle only
        else a = (row == col) ? 1.f : 0.f;
        const float v = a - acc[e];
        if (t == 0) Ds[lr * CH_LDD + li] = v;
        else Wb[(size_t)row * Np + col] = v;
      }
    }
    __syncthreads();
    if (wave == 0) {  // 32 x 32 diagonal block, lane li = row li (both halves of the wave compute the same values)
      float r[CH_NB];
      int lv = li;  // opaque per panel: the 64 lane masks (lv > j, lv == j) are otherwise hoisted out of the panel loop
      asm volatile("" : "+v"(lv));
#pragma unroll
      for (int c = 0; c < CH_NB; ++c) r[c] = Ds[li * CH_LDD + c];
      if (col0 > 0) {
        const int rr = col0 + li;
        const float d0 = (float)((rr < N ? (double)Ab[(size_t)rr * N + rr] : 1.0) - ds[rr]);
#pragma unroll
        for (int c = 0; c < CH_NB; ++c) r[c] = (lv == c) ? d0 : r[c];
      }
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) {
        const float piv = lane_bcast(r[j], j);
        if (!(piv > 0.f) && first_bad == 0 && col0 + j < N) first_bad = col0 + j + 1;
        const float s = sqrtf(piv);
        const float inv = 1.0f / s;
        r[j] = (lv > j) ? r[j] * inv : ((lv == j) ? s : 0.f);
        if (lane == 0) dinv[j] = inv;
#pragma unroll
        for (int c = j + 1; c < CH_NB; ++c) {
          const float lcj = lane_bcast(r[j], c);
          r[c] = fmaf(-r[j], lcj, r[c]);
        }
        __builtin_amdgcn_sched_barrier(0);  // keeps one column's broadcasts (SGPRs) live at a time: no SGPR spills
      }
      float dg = 1.f;
#pragma unroll
      for (int c = 0; c < CH_NB; ++c) dg = (lv == c) ? r[c] : dg;
      if (col0 + li < N) ld += log((double)dg);
      if (h == 0) {
#pragma unroll
        for (int c = 0; c < CH_NB; ++c) {
          Ds[li * CH_LDD + c] = r[c];
          Wb[(size_t)(col0 + li) * Np + col0 + c] = r[c];
        }
      }
    }
    __syncthreads();
    for (int rr = col0 + CH_NB + tid; rr < Np; rr += kThreads) {  // rows below the block: x L_kk^-T
      float x[CH_NB];
      float* wr = Wb + (size_t)rr * Np + col0;
      asm volatile("" ::: "memory");  // the block is re-read from LDS per row: hoisted, its 528 uniform values spill SGPRs
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(wr + 4 * q);
        x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) {
        float s = x[j];
#pragma unroll
        for (int c = 0; c < j; ++c) s = fmaf(-x[c], Ds[j * CH_LDD + c], s);
        x[j] = s * dinv[j];
      }
      double sq = 0.0;
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) sq += (double)x[j] * (double)x[j];
      ds[rr] += sq;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        *reinterpret_cast<float4*>(wr + 4 * q) = make_float4(x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
    }
    __syncthreads();
  }
  float* Lb = Lout + (size_t)b * N * N;
  for (int idx = tid; idx < N * N; idx += kThreads) {
    const int r = idx / N, c = idx - r * N;
    Lb[idx] = (c <= r) ? Wb[(size_t)r * Np + c] : 0.f;
  }
  if (wave == 0) {
    for (int off = 16; off > 0; off >>= 1) ld += __shfl_xor(ld, off, 32);  // fixed tree over the 32 row classes
    if (tid == 0) {
      info[b] = first_bad;
      if (logdet) logdet[b] = 2.0 * ld;
    }
  }
}

// ------------------------------------------------------------------------------------------------------ substitution
template <int CB>
struct TsLayout {
  static constexpr int LDX = CB == 16 ? 20 : CB;  // row stride of the right-hand-side tile (float4 rows for CB >= 4)
  static size_t bytes(int Np) {
    return sizeof(float) * ((size_t)Np * LDX + TS_KS * CH_LDD + CH_NB * CH_LDD + 8 * CH_NB * CB + CH_NB);
  }
};

// One sweep over the blocks of 32 rows: forward (bwd = 0) for an effectively lower matrix M, backward for an upper one;
// M[i][k] = T[i][k] (tr = 0) or T[k][i] (tr = 1).  X [Np, LDX] in LDS is solved in place.
template <int CB>
__device__ __forceinline__ void ts_sweep(const float* __restrict__ Tb, float* X, float* S, float* D, float* red, int N,
                                         int Np, bool bwd, bool tr) {
  constexpr int LDX = TsLayout<CB>::LDX;
  const int tid = threadIdx.x, i = tid & 31, g = tid >> 5;
  const int nblk = Np / CH_NB;
  for (int bi = 0; bi < nblk; ++bi) {
    const int r0 = CH_NB * (bwd ? nblk - 1 - bi : bi);
    const int klo = bwd ? r0 + CH_NB : 0, khi = bwd ? Np : r0;
    float acc[CB];
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) acc[cc] = 0.f;
    for (int k0 = klo; k0 < khi; k0 += TS_KS) {
      const int kend = min(TS_KS, khi - k0);
#pragma unroll 4
      for (int u = 0; u < 16; ++u) {
        const int idx = tid + kThreads * u;
        int k, ii, gr, gc;
        if (!tr) { k = idx & (TS_KS - 1); ii = idx >> 7; gr = r0 + ii; gc = k0 + k; }
        else { ii = idx & 31; k = idx >> 5; gr = k0 + k; gc = r0 + ii; }
        float v = 0.f;
        if (k < kend && gr < N && gc < N) v = Tb[(size_t)gr * N + gc];
        S[k * CH_LDD + ii] = v;
      }
      __syncthreads();
      const int kk1 = min(16 * g + 16, kend);
      for (int kk = 16 * g; kk < kk1; ++kk) {
        const float m = S[kk * CH_LDD + i];
        const float* xr = X + (size_t)(k0 + kk) * LDX;
        if constexpr (CB % 4 == 0) {
#pragma unroll
          for (int q = 0; q < CB / 4; ++q) {
            const float4 x4 = *reinterpret_cast<const float4*>(xr + 4 * q);
            acc[4 * q] = fmaf(m, x4.x, acc[4 * q]);
            acc[4 * q + 1] = fmaf(m, x4.y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(m, x4.z, acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(m, x4.w, acc[4 * q + 3]);
          }
        } else {
#pragma unroll
          for (int cc = 0; cc < CB; ++cc) acc[cc] = fmaf(m, xr[cc], acc[cc]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) red[(g * CH_NB + i) * CB + cc] = acc[cc];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // the diagonal block, D[k][i] = M[r0 + i][r0 + k]; identity beyond N
      const int idx = tid + kThreads * u;
      int k, ii, gr, gc;
      if (!tr) { k = idx & 31; ii = idx >> 5; gr = r0 + ii; gc = r0 + k; }
      else { ii = idx & 31; k = idx >> 5; gr = r0 + k; gc = r0 + ii; }
      D[k * CH_LDD + ii] = (gr < N && gc < N) ? Tb[(size_t)gr * N + gc] : ((ii == k) ? 1.f : 0.f);
    }
    __syncthreads();
    for (int idx = tid; idx < CH_NB * CB; idx += kThreads) {
      const int ii = idx / CB, cc = idx - ii * CB;
      float s = 0.f;
#pragma unroll
      for (int gg = 0; gg < 8; ++gg) s += red[(gg * CH_NB + ii) * CB + cc];
      X[(size_t)(r0 + ii) * LDX + cc] -= s;
    }
    float* dinv = red + 8 * CH_NB * CB;  // 1 / M_kk of the block, once per block instead of a division per step
    if (tid < CH_NB) dinv[tid] = 1.0f / D[tid * CH_LDD + tid];
    __syncthreads();
    for (int cc = g; cc < CB; cc += 8) {  // a half-wave per column, lane i = row r0 + i
      float x = X[(size_t)(r0 + i) * LDX + cc];
      for (int s = 0; s < CH_NB; ++s) {
        const int k = bwd ? CH_NB - 1 - s : s;
        const float xk = __shfl(x, k, 32) * dinv[k];
        if (i == k) x = xk;
        else if (bwd ? (i < k) : (i > k)) x = fmaf(-D[k * CH_LDD + i], xk, x);
      }
      X[(size_t)(r0 + i) * LDX + cc] = x;
    }
    __syncthreads();
  }
}

// mode 0: out = M^-1 rhs with M = T or T^T (trans) of a lower or upper (upper) factor; mode 1: (T T^T)^-1 rhs for a
// lower factor, (T^T T)^-1 rhs for an upper one -- the forward result never leaves LDS.
template <int CB>
__global__ __launch_bounds__(kThreads) void k_tri_solve(const float* __restrict__ T, const float* __restrict__ rhs,
                                                        float* __restrict__ out, float* __restrict__ sumsq, int N,
                                                        int Np, int c, int mode, int upper, int trans) {
  constexpr int LDX = TsLayout<CB>::LDX;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* X = sm;
  float* S = X + (size_t)Np * LDX;
  float* D = S + TS_KS * CH_LDD;
  float* red = D + CH_NB * CH_LDD;
  const int b = blockIdx.x, c0 = CB * blockIdx.y, cw = min(CB, c - c0), tid = threadIdx.x;
  const float* Tb = T + (size_t)b * N * N;
  const float* rb = rhs + (size_t)b * N * c + c0;
  float* ob = out + (size_t)b * N * c + c0;
  for (int idx = tid; idx < Np * CB; idx += kThreads) {
    const int r = idx / CB, cc = idx - r * CB;
    X[(size_t)r * LDX + cc] = (r < N && cc < cw) ? rb[(size_t)r * c + cc] : 0.f;
  }
  __syncthreads();
  for (int pass = 0; pass <= mode; ++pass) {  // one sweep, or forward then backward for the Cholesky solve
    const bool bwd = mode ? pass == 1 : (upper != 0) != (trans != 0);
    const bool tr = mode ? (upper != 0) != (pass == 1) : trans != 0;
    ts_sweep<CB>(Tb, X, S, D, red, N, Np, bwd, tr);
  }
  for (int idx = tid; idx < N * CB; idx += kThreads) {
    const int r = idx / CB, cc = idx - r * CB;
    if (cc < cw) ob[(size_t)r * c + cc] = X[(size_t)r * LDX + cc];
  }
  if (sumsq) {
    const int i = tid & 31, g = tid >> 5;
    for (int cc = g; cc < cw; cc += 8) {
      double s = 0.0;
      for (int r = i; r < N; r += 32) {
        const double v = (double)X[(size_t)r * LDX + cc];
        s += v * v;
      }
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
      if (i == 0) sumsq[(size_t)b * c + c0 + cc] = (float)s;
    }
  }
}

template <int CB>
int ts_launch(const float* T, const float* rhs, float* out, float* sumsq, int64_t B, int N, int c, int mode, int upper,
              int trans, hipStream_t st) {
  const int Np = (N + CH_NB - 1) / CH_NB * CH_NB;
  const size_t lds = TsLayout<CB>::bytes(Np);
  if (lds > 64 * 1024)  // the opt-in beyond 64 KiB of dynamic LDS belongs to the current device: set it per launch
    LO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tri_solve<CB>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)B, (unsigned)((c + CB - 1) / CB));
  LO_PROF_BEGIN(mode ? "chol_solve" : "tri_solve", st);
  hipLaunchKernelGGL(k_tri_solve<CB>, grid, dim3(kThreads), lds, st, T, rhs, out, sumsq, N, Np, c, mode, upper, trans);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int ts_dispatch(const float* T, const float* rhs, float* out, float* sumsq, int64_t B, int64_t N, int64_t c, int mode,
                int upper, int trans, void* stream) {
  if (!T || !rhs || !out || B < 0 || N < 1 || c < 1) return LO_ERR_BADARG;
  if (N > kCholMaxN || B > 0x7fffffff || c > 16 * 65535) return LO_ERR_UNSUPPORTED;
  if (B == 0) return LO_OK;
  hipStream_t st = (hipStream_t)stream;
  if (c == 1) return ts_launch<1>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
  if (c <= 4) return ts_launch<4>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
  return ts_launch<16>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
}

// the workspace of lo_cholesky_f32 (Np: N rounded up to whole panels)
constexpr size_t kCholTail = 512;  // what the sizer reports beyond the layout
struct CholBufs { float* W; double* dsum; };  // the factor's working copy [B, Np, Np], fp64 row sums [B, Np]
CholBufs chol_layout(Arena& ar, int64_t B, int64_t Np) {
  return {ar.take<float>((size_t)B * Np * Np), ar.take<double>((size_t)B * Np)};
}
int chol_padded(int64_t N) { return (int)((N + CH_NB - 1) / CH_NB * CH_NB); }

}  // namespace
}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_cholesky_workspace_bytes(int64_t B, int64_t N) {
  if (B < 1 || N < 1 || N > kCholMaxN) return 0;
  return measured(kCholTail, [&](Arena& ar) { chol_layout(ar, B, chol_padded(N)); });
}

int lo_cholesky_f32(const float* A, float* L, int32_t* info, double* logdet, int64_t B, int64_t N, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!A || !L || !info || B < 0 || N < 1) return LO_ERR_BADARG;
  if (N > kCholMaxN || B > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  if (B == 0) return LO_OK;
  const int Np = chol_padded(N);
  Arena ar(ws, ws_bytes, kCholTail);
  auto [W, dsum] = chol_layout(ar, B, Np);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const int ldb = Np - CH_NB + 4;
  const size_t lds = sizeof(float) * (size_t)CH_NB * ldb;  // + 4352 bytes static
  if (lds > 64 * 1024)
    LO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_blocked),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipStream_t st = (hipStream_t)stream;
  LO_PROF_BEGIN("cholesky", st);
  hipLaunchKernelGGL(k_chol_blocked, dim3((unsigned)B), dim3(kThreads), lds, st, A, W, L, info, logdet, dsum, (int)N,
                     Np, ldb);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int lo_tri_solve_f32(const float* T, const float* rhs, float* out, float* sumsq, int64_t B, int64_t N, int64_t c,
                     int32_t upper, int32_t transpose, void* stream) {
  return ts_dispatch(T, rhs, out, sumsq, B, N, c, 0, upper, transpose, stream);
}

int lo_cholesky_solve_f32(const float* T, const float* rhs, float* out, int64_t B, int64_t N, int64_t c, int32_t upper,
                          void* stream) {
  return ts_dispatch(T, rhs, out, nullptr, B, N, c, 1, upper, 0, stream);
}

}  // extern "C"
