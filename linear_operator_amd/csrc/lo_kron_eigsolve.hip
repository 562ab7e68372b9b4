// lo_kron_eigsolve.hip -- y = scale o ((M1 (x) S2^T) z): one half of the closed-form inverse of a sum of two Kronecker
// products (reference: operators/sum_kronecker_linear_operator.py:42-66, the eigenbasis sandwich
//   (A (x) B + C (x) D)^-1 = (P_1 (x) P_2) diag(1 / (lambda_1 (x) lambda_2 + 1)) (P_1 (x) P_2)^T ;
//  DESIGN.md section 6k).  With Z the [n1, n2] view of a column of z (row index i1 n2 + i2):
//   Y = scale o (M1 (Z S2)),      M1 [n1, n1] the data factor (hundreds to thousands), S2 [n2, n2] the task factor.
// Two routes behind one entry point:
//   fused    n2 <= LO_KRON_EIG_MAX_SMALL: ONE launch.  W = Z S2 is never stored: the slab of W a workgroup needs next
//            (256 contraction indices x CT of the n2 c columns) is formed from Z and S2 while it is staged to LDS, M1 is
//            streamed with 16-byte row loads (one wave instruction = 1 KiB of one row, lanes stride over the contraction
//            index as in lo_dense.hip), and scale is applied where the row sums leave the wave reduce-scatter.
//   general  n2 > LO_KRON_EIG_MAX_SMALL: S2 is transposed into the workspace, the Kronecker matvec engines of
//            lo_kron.hip form (M1 (x) S2^T) z (matrix cores where they take the shape) and one kernel scales.
// Fixed-order sums, no float atomics: the same inputs give the same bits.
#include <algorithm>
#include <stdint.h>
#include <stdlib.h>

#include "lo_device.h"
#include "lo_internal.h"

namespace lo {

constexpr int KE_KS = kThreads;  // contraction indices per slab: one per thread when staged, four per lane when used

// floats of the W slab in LDS: lane block l holds W[4 l .. 4 l + 3][0 .. CT) (vector mode) followed by 4 floats of padding
// -- the lanes' ds_read_b128 start 4 CT + 4 dwords apart, which spreads every 16-lane group over all 64 banks
template <int CT>
constexpr int ke_lane_block() { return 4 * CT + 4; }

// CT: columns of W per pass (4 or 8); RW: rows of M1 per wave (4 or 8), a workgroup owns 4 RW consecutive rows.
//   vec != 0  (n1 % 4 == 0: every row of M1 starts 16-byte aligned): lane l owns contraction indices k0 + 4 l + jj
//   vec == 0  (any n1): lane l owns k0 + l + 64 jj, scalar loads, still coalesced
// Rows beyond n1 read row n1 - 1 and are not stored; contraction indices beyond n1 contribute zeros.
template <int CT, int RW>
__global__ __launch_bounds__(kThreads) void k_kron_eig_fused(const float* __restrict__ M1, const float* __restrict__ S2,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ z, float* __restrict__ y, int n1,
                                                              int n2, int c, int vec) {
  constexpr int LB = ke_lane_block<CT>();
  constexpr int NA = RW * CT;  // accumulators per lane
  __shared__ __attribute__((aligned(16))) float wsl[64 * LB];
  __shared__ float s2s[LO_KRON_EIG_MAX_SMALL * LO_KRON_EIG_MAX_SMALL];
  const int b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int P = n2 * c;  // columns of W and of Y, p = i2 c + col
  const int row0 = (blockIdx.x * 4 + wave) * RW;
  const float* Mb = M1 + (size_t)b * n1 * n1;
  const float* zb = z + (size_t)b * n1 * P;
  float* yb = y + (size_t)b * n1 * P;
  for (int e = threadIdx.x; e < n2 * n2; e += kThreads) s2s[e] = S2[(size_t)b * n2 * n2 + e];
  const float* mr[RW];
#pragma unroll
  for (int u = 0; u < RW; ++u) mr[u] = Mb + (size_t)min(row0 + u, n1 - 1) * n1;
  // the slab entry this thread forms: contraction index k0 + t, stored where the lane that owns it reads it
  const int t = threadIdx.x;
  float* wst = vec ? &wsl[(t >> 2) * LB + (t & 3) * CT] : &wsl[(t & 63) * LB + (t >> 6) * CT];
  const float* wld = &wsl[lane * LB];

  for (int p0 = 0; p0 < P; p0 += CT) {
    float acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    // (column p0 + q of W: task index and right-hand-side column, fixed over the slabs)
    int wi2[CT], wcol[CT];
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int p = min(p0 + q, P - 1);
      wi2[q] = p / c;
      wcol[q] = p - wi2[q] * c;
    }
    for (int k0 = 0; k0 < n1; k0 += KE_KS) {
      // M1 first: the loads are in flight while the slab of W is formed
      float a[RW][4];
      if (vec) {
        const int k = k0 + 4 * lane;
#pragma unroll
        for (int u = 0; u < RW; ++u) {
          const float4 a4 = (k < n1) ? *reinterpret_cast<const float4*>(mr[u] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
          a[u][0] = a4.x; a[u][1] = a4.y; a[u][2] = a4.z; a[u][3] = a4.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < RW; ++u)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int k = k0 + lane + 64 * jj;
            a[u][jj] = (k < n1) ? mr[u][k] : 0.f;
          }
      }
      __syncthreads();  // the previous slab has been read (first pass: s2s is complete)
      {
        const int k = k0 + t;
        float w[CT];
#pragma unroll
        for (int q = 0; q < CT; ++q) w[q] = 0.f;
        if (k < n1) {
          const float* zr = zb + (size_t)k * P;  // Z[k, j2, col] at zr[j2 c + col]
          for (int j2 = 0; j2 < n2; ++j2) {
#pragma unroll
            for (int q = 0; q < CT; ++q) w[q] = fmaf(zr[j2 * c + wcol[q]], s2s[j2 * n2 + wi2[q]], w[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < CT; ++q) wst[q] = (p0 + q < P) ? w[q] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        float wv[CT];
#pragma unroll
        for (int q4 = 0; q4 < CT / 4; ++q4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wld + jj * CT + 4 * q4);
          wv[4 * q4] = w4.x; wv[4 * q4 + 1] = w4.y; wv[4 * q4 + 2] = w4.z; wv[4 * q4 + 3] = w4.w;
        }
#pragma unroll
        for (int u = 0; u < RW; ++u)
#pragma unroll
          for (int q = 0; q < CT; ++q) acc[u * CT + q] = fmaf(a[u][jj], wv[q], acc[u * CT + q]);
      }
    }
    // wave reduce-scatter: lane l ends with the sum of accumulator l >> SH (lo_group_reduce.h)
    halving_steps<NA, 32, NA>(acc, lane);
    constexpr int SH = (NA == 64) ? 0 : (NA == 32) ? 1 : 2;
    static_assert(NA == 64 || NA == 32 || NA == 16, "one accumulator per 1, 2 or 4 lanes");
    if ((lane & ((1 << SH) - 1)) == 0) {
      const int comp = lane >> SH, u = comp / CT, q = comp % CT;
      const int row = row0 + u, p = p0 + q;
      if (row < n1 && p < P) {
        float v = acc[0];
        if (scale) v *= scale[(size_t)b * n1 * n2 + (size_t)row * n2 + p / c];
        yb[(size_t)row * P + p] = v;
      }
    }
  }
}

// S2 [B, n, n] -> its transpose (general route; n2 x n2 floats per member)
__global__ __launch_bounds__(kThreads) void k_kron_eig_transpose(const float* __restrict__ in, float* __restrict__ out,
                                                                  int n) {
  const size_t o = (size_t)blockIdx.y * n * n;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e < n * n) out[o + (size_t)(e % n) * n + e / n] = in[o + e];
}

// y[b, i, col] *= scale[b, i]
__global__ __launch_bounds__(kThreads) void k_kron_eig_scale(float* __restrict__ y, const float* __restrict__ scale,
                                                              size_t total, int c) {
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads)
    y[e] *= scale[e / c];
}

static bool ke_fused_shape(int64_t n2, int64_t c) {
  return n2 <= LO_KRON_EIG_MAX_SMALL && c <= LO_KRON_EIG_MAX_COLS && !getenv("LO_KRON_EIG_NO_FUSED");
}
// what the general route takes: the limits of the Kronecker matvec engines (int sizes, one grid slot per (member, column))
static bool ke_general_shape(int64_t B, int64_t n1, int64_t n2, int64_t c) {
  return n1 * n2 * c < ((int64_t)1 << 31) && n1 * n1 < ((int64_t)1 << 31) && B * c <= 65535 && B <= 65535;
}

struct KeGeneral {
  float *s2t, *tmp;
};
static void ke_general_layout(Arena& ar, int64_t B, int64_t n1, int64_t n2, int64_t c, KeGeneral* g) {
  const bool cols = kron_mfma_cols_ok((int)n1, (int)n2, c);
  g->s2t = ar.take<float>((size_t)B * n2 * n2);
  g->tmp = ar.take<float>((size_t)B * n1 * n2 * c * (cols ? 2 : 1));
}

static int ke_fused(const float* M1, const float* S2, const float* scale, const float* z, float* y, int64_t B, int n1,
                    int n2, int c, hipStream_t st) {
  const int P = n2 * c;
  // 32 rows per workgroup once that still gives two workgroups per CU, else 16 (small batches of one tall factor)
  const bool rw8 = B * ((n1 + 31) / 32) >= 512;
  const int rows = rw8 ? 32 : 16;
  const dim3 grid((unsigned)((n1 + rows - 1) / rows), (unsigned)B);
  const int vec = (n1 % 4 == 0 && (uintptr_t)M1 % 16 == 0) ? 1 : 0;  // 16-byte row loads need aligned rows
  LO_PROF_BEGIN("kron_eig_fused", st);
#define LO_KE(CT, RW) \
  hipLaunchKernelGGL((k_kron_eig_fused<CT, RW>), grid, dim3(kThreads), 0, st, M1, S2, scale, z, y, n1, n2, c, vec)
  if (P <= 4) {
    if (rw8) LO_KE(4, 8);
    else LO_KE(4, 4);
  } else {
    if (rw8) LO_KE(8, 8);
    else LO_KE(8, 4);
  }
#undef LO_KE
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_kron_eig_apply_workspace_bytes(int64_t B, int64_t n1, int64_t n2, int64_t c) {
  if (B < 1 || n1 < 1 || n2 < 1 || c < 1) return 0;
  if (ke_fused_shape(n2, c)) return (B <= 65535 && n1 * n2 * c < ((int64_t)1 << 31)) ? kPlanTail : 0;
  if (n2 <= LO_KRON_EIG_MAX_SMALL && !getenv("LO_KRON_EIG_NO_FUSED")) return 0;  // (too many columns: the caller composes)
  if (!ke_general_shape(B, n1, n2, c)) return 0;
  KeGeneral g;
  return measured(kPlanTail, [&](Arena& ar) { ke_general_layout(ar, B, n1, n2, c, &g); });
}

int lo_kron_eig_apply_f32(const float* M1, const float* S2, const float* scale, const float* z, float* y, int64_t B,
                          int64_t n1, int64_t n2, int64_t c, void* ws, size_t ws_bytes, void* stream) {
  if (!M1 || !S2 || !z || !y || B < 1 || n1 < 1 || n2 < 1 || c < 1) return LO_ERR_BADARG;
  const size_t need = lo_kron_eig_apply_workspace_bytes(B, n1, n2, c);
  if (need == 0) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (ke_fused_shape(n2, c)) return ke_fused(M1, S2, scale, z, y, B, (int)n1, (int)n2, (int)c, st);
  if (!ws || ws_bytes < need) return LO_ERR_WORKSPACE;
  Arena ar(ws, ws_bytes);
  KeGeneral g;
  ke_general_layout(ar, B, n1, n2, c, &g);
  if (!ar.ok) return LO_ERR_WORKSPACE;
  const int m1 = (int)n1, m2 = (int)n2;
  LO_PROF_BEGIN("kron_eig_transpose", st);
  hipLaunchKernelGGL(k_kron_eig_transpose, dim3((unsigned)((n2 * n2 + kThreads - 1) / kThreads), (unsigned)B),
                     dim3(kThreads), 0, st, S2, g.s2t, m2);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  int rc;
  if (kron_mfma_ok(m1, m2, c))
    rc = kron_matvec_mfma(M1, g.s2t, nullptr, LO_DIAG_NONE, z, g.tmp, y, nullptr, B, m1, m2, nullptr, st);
  else if (kron_mfma_cols_ok(m1, m2, c))
    rc = kron_matvec_mfma_cols(M1, g.s2t, nullptr, LO_DIAG_NONE, z, g.tmp, g.tmp + (size_t)B * n1 * n2 * c, y, B, m1, m2,
                               c, nullptr, st);
  else
    rc = kron_matvec(M1, g.s2t, z, g.tmp, y, B, m1, m2, c, nullptr, st);
  if (rc) return rc;
  if (scale) {
    const size_t total = (size_t)B * n1 * n2 * c;
    const unsigned blocks = (unsigned)std::min<size_t>((total + kThreads - 1) / kThreads, 2048);
    LO_PROF_BEGIN("kron_eig_scale", st);
    hipLaunchKernelGGL(k_kron_eig_scale, dim3(blocks), dim3(kThreads), 0, st, y, scale, total, (int)c);
    LO_PROF_END(st);
    LO_LAUNCH_CHECK();
  }
  return LO_OK;
}

}  // extern "C"
