// lo_chol_f64.hip -- the exact small-N path (N <= 1024) in fp64: batched lower Cholesky, triangular solves and the
// two-sided Cholesky solve, the float64 twin of lo_chol.hip (same entry-point semantics, one workgroup per member, per
// member and column block for the solves).  Every operand, product and sum is float64.
//
// lo_cholesky_f64: blocked LEFT-looking factorisation, panels of 32 columns, in a padded workspace copy W [Np, Np],
// Np = N rounded up to 32, initialised to blockdiag(tril(A), I) so that no loop has a ragged edge.  Per panel:
//   1. the 32 finished rows L[col0 .. col0+31, 0 .. col0) are the B operand every row tile shares.  In doubles they do
//      not fit (32 x 996 x 8 = 255 KB at N = 1024), so they STREAM through LDS in k-slabs of 256 columns;
//   2. per slab every wave takes row tiles of 32: W[tile, panel] -= L[tile, slab] L[panel, slab]^T, four 16 x 16
//      accumulators on v_mfma_f64_16x16x4_f64 (A operand straight from W, 64 contiguous bytes per lane and k-step of
//      32; lane (i = l % 16, g = l / 16) owns k = 8 g .. 8 g + 7 of the step for both operands);
//   3. wave 0 factorises the 32 x 32 diagonal block in registers (lane = row, columns broadcast through LDS);
//   4. one thread per row below it substitutes against the block (broadcast LDS reads).
// The pivots are float64, so the log-determinant comes from them directly (no separate row-sum buffer).
// LDS at N = 1024: slab [32][258] doubles = 66,048 B dynamic + 8,960 B static (diagonal block [32][33], 1 / L_jj,
// a column of the block) = 75,008 B, two workgroups per compute unit; smaller N take a slab of Np - 32 columns.
//
// lo_tri_solve_f64 / lo_cholesky_solve_f64: blocked substitution, blocks of 32 rows, the N x CB tile of right-hand
// sides resident in LDS for the whole launch (both sweeps of the Cholesky solve included), CB = 1, 4 or 8.  Per block
// the update X[blk] -= M[blk, done] X[done] streams M in slabs of 128 through LDS, each of the 8 half-waves owning every
// eighth k of the slab for all CB columns, a fixed-order sum of the 8 partials, then the 32 x 32 diagonal block is solved
// by a half-wave per column.  LDS at N = 1024: CB = 8 124,416 B, CB = 4 83,456 B, CB = 1 52,736 B.
//
// Sums run in a fixed order, there is no atomic and no inter-workgroup communication: a member's result does not depend
// on the batch it is in, and repeats bit for bit.
#include "lo_internal.h"

namespace lo {
namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;
constexpr int DC_NB = 32;       // panel width / block rows
constexpr int DC_LDD = 33;      // row stride of the 32 x 32 diagonal block in LDS
constexpr int DC_KS = 256;      // k-slab of the finished panel rows
constexpr int DT_KS = 128;      // k-slab of the substitution update
constexpr int kChol64MaxN = 1024;

// ---------------------------------------------------------------------------------------------------- factorisation
// v_mfma_f64_16x16x4_f64: lane l supplies A[i = l % 16][kk = l / 16] and B[kk][j = l % 16]; result register r of lane l
// is D[4 r + l / 16][l % 16] (lo_precond.hip).  Which k a lane group contributes is free as long as A and B agree.
// (two waves per SIMD: within 256 registers the kernel has no scratch, and two workgroups share a compute unit)
__global__ __launch_bounds__(kThreads, 2) void k_chol_blocked_f64(const double* __restrict__ A, double* __restrict__ W,
                                                               double* __restrict__ Lout, int* __restrict__ info,
                                                               double* __restrict__ logdet, int N, int Np, int ldb) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  __shared__ double Ds[DC_NB * DC_LDD];  // [32][33]    diagonal block
  __shared__ double dinv[DC_NB];         // [32]        1 / L_jj of the block
  __shared__ double cb[DC_NB];           // [32]        the block's current column, broadcast to its rows
  double* Bs = smd;                      // [32][ldb]   a k-slab of the panel's finished rows, k-contiguous
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
  const double* Ab = A + (size_t)b * N * N;
  double* Wb = W + (size_t)b * Np * Np;
  // W = blockdiag(tril(A), I).  One workgroup has few loads in flight: every copy loop below issues 8 independent loads
  // per thread before the first store, or it runs at one memory latency per element.
  {
    const int hp = Np >> 1, pairs = Np * hp;
    for (int base = 0; base < pairs; base += kThreads * 8) {
      double2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + tid + kThreads * u;
        const int r = idx / hp, c = 2 * (idx - r * hp);
        double x = (r == c) ? 1.0 : 0.0, y = 0.0;  // (the pair starts at an even column: r == c + 1 never pads)
        if (idx < pairs && r < N) {
          if (c < N) x = (c <= r) ? Ab[(size_t)r * N + c] : 0.0;
          if (c + 1 < N) y = (c + 1 <= r) ? Ab[(size_t)r * N + c + 1] : 0.0;
        }
        if (r == c + 1 && r >= N) y = 1.0;
        v[u] = make_double2(x, y);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + tid + kThreads * u;
        if (idx < pairs) *reinterpret_cast<double2*>(Wb + 2 * (size_t)idx) = v[u];
      }
    }
  }
  __syncthreads();
  int first_bad = 0;  // wave 0 only (uniform)
  double ld = 0.0;    // wave 0 only: lane li sums log L_rr over its rows r = 32 p + li

  for (int col0 = 0; col0 < Np; col0 += DC_NB) {
    const int tiles = (Np - col0) / DC_NB;
    for (int s0 = 0; s0 < col0; s0 += DC_KS) {
      const int kw = min(DC_KS, col0 - s0), q2 = kw >> 1;
      for (int base = 0; base < DC_NB * q2; base += kThreads * 8) {  // (DC_NB * q2 is a multiple of 256)
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = min(base + tid + kThreads * u, DC_NB * q2 - 1), j = idx / q2, q = idx - j * q2;
          v[u] = *reinterpret_cast<const double2*>(Wb + (size_t)(col0 + j) * Np + s0 + 2 * q);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = base + tid + kThreads * u, j = idx / q2, q = idx - j * q2;
          if (idx < DC_NB * q2) *reinterpret_cast<double2*>(Bs + j * ldb + 2 * q) = v[u];
        }
      }
      __syncthreads();
      for (int t = wave; t < tiles; t += 4) {
        const int r0 = col0 + DC_NB * t;
        f64x4 acc[2][2];
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
#pragma unroll
          for (int ch = 0; ch < 2; ++ch) acc[rh][ch] = f64x4{0.0, 0.0, 0.0, 0.0};
        const double* ap = Wb + (size_t)(r0 + i) * Np + s0 + 8 * g;
        const double* bp = Bs + i * ldb + 8 * g;
        // the A operand of step k0 + 32 is requested before the 32 MFMAs of step k0 (a wave is alone on its SIMD)
        double2 a0[4], a1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a0[q] = *reinterpret_cast<const double2*>(ap + 2 * q);
          a1[q] = *reinterpret_cast<const double2*>(ap + (size_t)16 * Np + 2 * q);
        }
        for (int k0 = 0; k0 < kw; k0 += 32) {
          double2 n0[4], n1[4], b0[4], b1[4];
          const int kn = (k0 + 32 < kw) ? k0 + 32 : k0;  // the last step re-reads itself: no branch, in bounds
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            n0[q] = *reinterpret_cast<const double2*>(ap + kn + 2 * q);
            n1[q] = *reinterpret_cast<const double2*>(ap + (size_t)16 * Np + kn + 2 * q);
            b0[q] = *reinterpret_cast<const double2*>(bp + k0 + 2 * q);
            b1[q] = *reinterpret_cast<const double2*>(bp + 16 * ldb + k0 + 2 * q);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q].x, b0[q].x, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q].x, b1[q].x, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[q].x, b0[q].x, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[q].x, b1[q].x, acc[1][1], 0, 0, 0);
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q].y, b0[q].y, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q].y, b1[q].y, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[q].y, b0[q].y, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[q].y, b1[q].y, acc[1][1], 0, 0, 0);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) { a0[q] = n0[q]; a1[q] = n1[q]; }
        }
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
#pragma unroll
          for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              double* w = Wb + (size_t)(r0 + 16 * rh + 4 * e + g) * Np + col0 + 16 * ch + i;
              *w -= acc[rh][ch][e];
            }
      }
      __syncthreads();
    }
    if (wave == 0) {  // 32 x 32 diagonal block, lane li = row li (both halves of the wave compute the same values)
      const int li = lane & 31, h = lane >> 5;
      double r[DC_NB];
      int lv = li;  // opaque per panel: the 64 lane masks (lv > j, lv == j) are otherwise hoisted out of the panel loop
      asm volatile("" : "+v"(lv));
      double* wr = Wb + (size_t)(col0 + li) * Np + col0;
#pragma unroll
      for (int q = 0; q < DC_NB / 2; ++q) {
        const double2 v = *reinterpret_cast<const double2*>(wr + 2 * q);
        r[2 * q] = v.x; r[2 * q + 1] = v.y;
      }
#pragma unroll
      for (int j = 0; j < DC_NB; ++j) {
        // column j is broadcast through LDS (one write, uniform-address reads): as v_readlane pairs a column's 31
        // doubles are 62 SGPRs and spill.  One wave: its LDS operations complete in order, no barrier is needed.
        cb[li] = r[j];
        const double piv = cb[j];
        if (!(piv > 0.0) && first_bad == 0 && col0 + j < N) first_bad = col0 + j + 1;
        const double s = sqrt(piv);
        const double inv = 1.0 / s;
        const double lj = r[j] * inv;
        r[j] = (lv > j) ? lj : ((lv == j) ? s : 0.0);
        if (lane == 0) dinv[j] = inv;
#pragma unroll
        for (int c = j + 1; c < DC_NB; ++c) {
          r[c] = fma(-lj, cb[c] * inv, r[c]);  // cb[c] * inv: row c's L_cj, same bits
          // pinned to its column: r[c] is consumed only at column c, and a deferred update keeps cb[c] * inv of every
          // earlier column live until then (spills)
          asm volatile("" : "+v"(r[c]));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      double dg = 1.0;
#pragma unroll
      for (int c = 0; c < DC_NB; ++c) dg = (lv == c) ? r[c] : dg;
      if (col0 + li < N) ld += log(dg);
      if (h == 0) {
#pragma unroll
        for (int c = 0; c < DC_NB; ++c) Ds[li * DC_LDD + c] = r[c];
#pragma unroll
        for (int q = 0; q < DC_NB / 2; ++q) *reinterpret_cast<double2*>(wr + 2 * q) = make_double2(r[2 * q], r[2 * q + 1]);
      }
    }
    __syncthreads();
    for (int rr = col0 + DC_NB + tid; rr < Np; rr += kThreads) {  // rows below the block: x L_kk^-T
      double x[DC_NB];
      double* wr = Wb + (size_t)rr * Np + col0;
      asm volatile("" ::: "memory");  // the block is re-read from LDS per row: hoisted, its 528 uniform values spill
#pragma unroll
      for (int q = 0; q < DC_NB / 2; ++q) {
        const double2 v = *reinterpret_cast<const double2*>(wr + 2 * q);
        x[2 * q] = v.x; x[2 * q + 1] = v.y;
      }
#pragma unroll
      for (int j = 0; j < DC_NB; ++j) {
        double s = x[j];
#pragma unroll
        for (int c = 0; c < j; ++c) s = fma(-x[c], Ds[j * DC_LDD + c], s);
        x[j] = s * dinv[j];
      }
#pragma unroll
      for (int q = 0; q < DC_NB / 2; ++q) *reinterpret_cast<double2*>(wr + 2 * q) = make_double2(x[2 * q], x[2 * q + 1]);
    }
    __syncthreads();
  }
  double* Lb = Lout + (size_t)b * N * N;
  for (int base = 0; base < N * N; base += kThreads * 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + tid + kThreads * u, r = idx / N, c = idx - r * N;
      v[u] = (idx < N * N && c <= r) ? Wb[(size_t)r * Np + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + tid + kThreads * u;
      if (idx < N * N) Lb[idx] = v[u];
    }
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
struct Ts64Layout {
  static constexpr int LDX = CB;  // row stride of the right-hand-side tile (16-byte rows for CB >= 2)
  static size_t bytes(int Np) {
    return sizeof(double) * ((size_t)Np * LDX + DT_KS * DC_LDD + DC_NB * DC_LDD + 8 * DC_NB * CB + DC_NB);
  }
};

// One sweep over the blocks of 32 rows: forward (bwd = 0) for an effectively lower matrix M, backward for an upper one;
// M[i][k] = T[i][k] (tr = 0) or T[k][i] (tr = 1).  X [Np, LDX] in LDS is solved in place.
template <int CB>
__device__ __forceinline__ void ts64_sweep(const double* __restrict__ Tb, double* X, double* S, double* D, double* red,
                                           int N, int Np, bool bwd, bool tr) {
  constexpr int LDX = Ts64Layout<CB>::LDX;
  const int tid = threadIdx.x, i = tid & 31, g = tid >> 5;
  const int nblk = Np / DC_NB;
  for (int bi = 0; bi < nblk; ++bi) {
    const int r0 = DC_NB * (bwd ? nblk - 1 - bi : bi);
    const int klo = bwd ? r0 + DC_NB : 0, khi = bwd ? Np : r0;
    double acc[CB];
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) acc[cc] = 0.0;
    for (int k0 = klo; k0 < khi; k0 += DT_KS) {
      const int kend = min(DT_KS, khi - k0);
#pragma unroll 4
      for (int u = 0; u < 16; ++u) {
        const int idx = tid + kThreads * u;
        int k, ii, gr, gc;
        if (!tr) { k = idx & (DT_KS - 1); ii = idx >> 7; gr = r0 + ii; gc = k0 + k; }
        else { ii = idx & 31; k = idx >> 5; gr = k0 + k; gc = r0 + ii; }
        double v = 0.0;
        if (k < kend && gr < N && gc < N) v = Tb[(size_t)gr * N + gc];
        S[k * DC_LDD + ii] = v;
      }
      __syncthreads();
      // half-wave g owns k = g, g + 8, ...: the two halves of a wave read neighbouring rows of X (different banks)
      for (int kk = g; kk < kend; kk += 8) {
        const double m = S[kk * DC_LDD + i];
        const double* xr = X + (size_t)(k0 + kk) * LDX;
        if constexpr (CB % 2 == 0) {
#pragma unroll
          for (int q = 0; q < CB / 2; ++q) {
            const double2 x2 = *reinterpret_cast<const double2*>(xr + 2 * q);
            acc[2 * q] = fma(m, x2.x, acc[2 * q]);
            acc[2 * q + 1] = fma(m, x2.y, acc[2 * q + 1]);
          }
        } else {
#pragma unroll
          for (int cc = 0; cc < CB; ++cc) acc[cc] = fma(m, xr[cc], acc[cc]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int cc = 0; cc < CB; ++cc) red[(g * DC_NB + i) * CB + cc] = acc[cc];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // the diagonal block, D[k][i] = M[r0 + i][r0 + k]; identity beyond N
      const int idx = tid + kThreads * u;
      int k, ii, gr, gc;
      if (!tr) { k = idx & 31; ii = idx >> 5; gr = r0 + ii; gc = r0 + k; }
      else { ii = idx & 31; k = idx >> 5; gr = r0 + k; gc = r0 + ii; }
      D[k * DC_LDD + ii] = (gr < N && gc < N) ? Tb[(size_t)gr * N + gc] : ((ii == k) ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int idx = tid; idx < DC_NB * CB; idx += kThreads) {
      const int ii = idx / CB, cc = idx - ii * CB;
      double s = 0.0;
#pragma unroll
      for (int gg = 0; gg < 8; ++gg) s += red[(gg * DC_NB + ii) * CB + cc];
      X[(size_t)(r0 + ii) * LDX + cc] -= s;
    }
    double* dinv = red + 8 * DC_NB * CB;  // 1 / M_kk of the block, once per block instead of a division per step
    if (tid < DC_NB) dinv[tid] = 1.0 / D[tid * DC_LDD + tid];
    __syncthreads();
    for (int cc = g; cc < CB; cc += 8) {  // a half-wave per column, lane i = row r0 + i
      double x = X[(size_t)(r0 + i) * LDX + cc];
      for (int s = 0; s < DC_NB; ++s) {
        const int k = bwd ? DC_NB - 1 - s : s;
        const double xk = __shfl(x, k, 32) * dinv[k];
        if (i == k) x = xk;
        else if (bwd ? (i < k) : (i > k)) x = fma(-D[k * DC_LDD + i], xk, x);
      }
      X[(size_t)(r0 + i) * LDX + cc] = x;
    }
    __syncthreads();
  }
}

// mode 0: out = M^-1 rhs with M = T or T^T (trans) of a lower or upper (upper) factor; mode 1: (T T^T)^-1 rhs for a
// lower factor, (T^T T)^-1 rhs for an upper one -- the forward result never leaves LDS.
template <int CB>
__global__ __launch_bounds__(kThreads) void k_tri_solve_f64(const double* __restrict__ T, const double* __restrict__ rhs,
                                                            double* __restrict__ out, double* __restrict__ sumsq, int N,
                                                            int Np, int c, int mode, int upper, int trans) {
  constexpr int LDX = Ts64Layout<CB>::LDX;
  extern __shared__ __attribute__((aligned(16))) double smd[];
  double* X = smd;
  double* S = X + (size_t)Np * LDX;
  double* D = S + DT_KS * DC_LDD;
  double* red = D + DC_NB * DC_LDD;
  const int b = blockIdx.x, c0 = CB * blockIdx.y, cw = min(CB, c - c0), tid = threadIdx.x;
  const double* Tb = T + (size_t)b * N * N;
  const double* rb = rhs + (size_t)b * N * c + c0;
  double* ob = out + (size_t)b * N * c + c0;
  for (int idx = tid; idx < Np * CB; idx += kThreads) {
    const int r = idx / CB, cc = idx - r * CB;
    X[(size_t)r * LDX + cc] = (r < N && cc < cw) ? rb[(size_t)r * c + cc] : 0.0;
  }
  __syncthreads();
  for (int pass = 0; pass <= mode; ++pass) {  // one sweep, or forward then backward for the Cholesky solve
    const bool bwd = mode ? pass == 1 : (upper != 0) != (trans != 0);
    const bool tr = mode ? (upper != 0) != (pass == 1) : trans != 0;
    ts64_sweep<CB>(Tb, X, S, D, red, N, Np, bwd, tr);
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
        const double v = X[(size_t)r * LDX + cc];
        s = fma(v, v, s);
      }
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
      if (i == 0) sumsq[(size_t)b * c + c0 + cc] = s;
    }
  }
}

template <int CB>
int ts64_launch(const double* T, const double* rhs, double* out, double* sumsq, int64_t B, int N, int c, int mode,
                int upper, int trans, hipStream_t st) {
  const int Np = (N + DC_NB - 1) / DC_NB * DC_NB;
  const size_t lds = Ts64Layout<CB>::bytes(Np);
  if (lds > 64 * 1024)  // the opt-in beyond 64 KiB of dynamic LDS belongs to the current device: set it per launch
    LO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tri_solve_f64<CB>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)B, (unsigned)((c + CB - 1) / CB));
  LO_PROF_BEGIN(mode ? "chol_solve_f64" : "tri_solve_f64", st);
  hipLaunchKernelGGL(k_tri_solve_f64<CB>, grid, dim3(kThreads), lds, st, T, rhs, out, sumsq, N, Np, c, mode, upper,
                     trans);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int ts64_dispatch(const double* T, const double* rhs, double* out, double* sumsq, int64_t B, int64_t N, int64_t c,
                  int mode, int upper, int trans, void* stream) {
  if (!T || !rhs || !out || B < 0 || N < 1 || c < 1) return LO_ERR_BADARG;
  if (N > kChol64MaxN || B > 0x7fffffff || c > 8 * 65535) return LO_ERR_UNSUPPORTED;
  if (B == 0) return LO_OK;
  hipStream_t st = (hipStream_t)stream;
  if (c == 1) return ts64_launch<1>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
  if (c <= 4) return ts64_launch<4>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
  return ts64_launch<8>(T, rhs, out, sumsq, B, (int)N, (int)c, mode, upper, trans, st);
}

// the workspace of lo_cholesky_f64 (Np: N rounded up to whole panels): the factor's working copy [B, Np, Np]
constexpr size_t kChol64Tail = 512;  // what the sizer reports beyond the layout
double* chol64_layout(Arena& ar, int64_t B, int64_t Np) { return ar.take<double>((size_t)B * Np * Np); }
int chol64_padded(int64_t N) { return (int)((N + DC_NB - 1) / DC_NB * DC_NB); }

}  // namespace
}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_cholesky_f64_workspace_bytes(int64_t B, int64_t N) {
  if (B < 1 || N < 1 || N > kChol64MaxN) return 0;
  return measured(kChol64Tail, [&](Arena& ar) { chol64_layout(ar, B, chol64_padded(N)); });
}

int lo_cholesky_f64(const double* A, double* L, int32_t* info, double* logdet, int64_t B, int64_t N, void* ws,
                    size_t ws_bytes, void* stream) {
  if (!A || !L || !info || B < 0 || N < 1) return LO_ERR_BADARG;
  if (N > kChol64MaxN || B > 0x7fffffff) return LO_ERR_UNSUPPORTED;
  if (B == 0) return LO_OK;
  const int Np = chol64_padded(N);
  Arena ar(ws, ws_bytes, kChol64Tail);
  double* W = chol64_layout(ar, B, Np);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  const int ldb = max(min(DC_KS, Np - DC_NB), DC_NB) + 2;  // rows 16 bytes apart in the banks: (2 ldb) % 64 == 4
  const size_t lds = sizeof(double) * (size_t)DC_NB * ldb;  // + 8960 bytes static
  if (lds > 64 * 1024)
    LO_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chol_blocked_f64),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipStream_t st = (hipStream_t)stream;
  LO_PROF_BEGIN("cholesky_f64", st);
  hipLaunchKernelGGL(k_chol_blocked_f64, dim3((unsigned)B), dim3(kThreads), lds, st, A, W, L, info, logdet, (int)N, Np,
                     ldb);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int lo_tri_solve_f64(const double* T, const double* rhs, double* out, double* sumsq, int64_t B, int64_t N, int64_t c,
                     int32_t upper, int32_t transpose, void* stream) {
  return ts64_dispatch(T, rhs, out, sumsq, B, N, c, 0, upper, transpose, stream);
}

int lo_cholesky_solve_f64(const double* T, const double* rhs, double* out, int64_t B, int64_t N, int64_t c,
                          int32_t upper, void* stream) {
  return ts64_dispatch(T, rhs, out, nullptr, B, N, c, 1, upper, 0, stream);
}

}  // extern "C"
