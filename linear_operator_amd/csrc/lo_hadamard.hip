// lo_hadamard.hip -- the Hadamard product of two roots, (F F^T) o (G G^T), on the fp32 matrix cores
// (mul_linear_operator.py:54-80 and :91-126 of the reference, LO_OP_HADAMARD_DIAG of lo_amd.h).
//
//   y[:, t] = rowdot(F, G M_t^T) + d o v_t,      M_t = F^T diag(v_t) G   [p x q]
//
// Phase A (contract, k_hd_contract): a workgroup takes a chunk of rows of one member and forms partial M_t for up to
//   four (t, 32-column block of G) tasks with v_mfma_f32_32x32x2_f32; the rows are staged 32 at a time in LDS, the
//   operand v_t o G is formed in registers.  Partials [B, S', T, QP, PP] go to the workspace.
// Reduce (k_hd_reduce): M [B, T, QP, PP] = sum over the S' partials in ascending order (M stored as M_t^T: the i index
//   of F innermost), and for the backward pass also the transposed copy [B, T, PP, QP].
// Phase B (expand, k_hd_expand): a workgroup stages 64 rows of F and G in LDS, forms W = M_t G_rows^T on the matrix
//   cores (A operand straight from the L2-resident M, B operand from LDS), takes the row-wise dot with F and adds d o v.
// Phase C (k_hd_grad): the gradients of sum_t u_t^T K v_t with respect to F and G from the contraction over the 2T
//   columns [v | u]:  dF = sum_t (u_t o G) M^v_t^T + (v_t o G) M^u_t^T,  dG likewise with F and M^T.
// Every sum runs in a fixed order and every output element is written by one plain store: results are bitwise the
// same from call to call (no float atomics).  p, q <= LO_HADAMARD_MAX_RANK.
#include <algorithm>

#include "lo_internal.h"

namespace lo {

using hd_f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kHdKB = 32;  // rows per LDS stage of phase A
constexpr int kHdRB = 64;  // rows per workgroup of phases B and C
constexpr int kHdTC = 8;   // columns per LDS round of phase B

struct HdShape {
  int64_t B, N, T;
  int p, q, PP, QP, PT, QT, PE, QE;
  int TW, RW, Z;  // tasks per workgroup of phase A, waves per task (row interleave), task groups
  int S, chunk;   // row chunks of phase A and their length
  int64_t tasks;
  size_t part_floats, m_floats;
};

static bool hd_shape(int64_t B, int64_t N, int64_t p, int64_t q, int64_t T, HdShape* s) {
  if (B < 1 || N < 1 || T < 1 || p < 1 || q < 1 || p > LO_HADAMARD_MAX_RANK || q > LO_HADAMARD_MAX_RANK) return false;
  if (B > 65535 || N > (int64_t)1 << 30) return false;
  s->B = B; s->N = N; s->T = T; s->p = (int)p; s->q = (int)q;
  s->PT = (int)((p + 31) / 32);
  s->QT = (int)((q + 31) / 32);
  s->PP = 32 * s->PT;
  s->QP = 32 * s->QT;
  s->PE = (int)((p + 1) & ~1);
  s->QE = (int)((q + 1) & ~1);
  s->tasks = T * s->QT;
  s->TW = s->tasks >= 4 ? 4 : (s->tasks >= 2 ? 2 : 1);
  s->RW = 4 / s->TW;
  const int64_t Z = (s->tasks + s->TW - 1) / s->TW;
  if (Z > 65535) return false;
  s->Z = (int)Z;
  // enough workgroups to fill the device (~512), chunks of at least 128 rows, at most 256 partials per task
  int64_t S = std::min<int64_t>(256, std::max<int64_t>(1, N / 128));
  S = std::min<int64_t>(S, std::max<int64_t>(1, (512 + Z * B - 1) / (Z * B)));
  int64_t chunk = (N + S - 1) / S;
  chunk = (chunk + kHdKB - 1) / kHdKB * kHdKB;
  s->chunk = (int)chunk;
  s->S = (int)((N + chunk - 1) / chunk);
  s->part_floats = (size_t)B * s->S * s->RW * T * s->QP * s->PP;
  s->m_floats = (size_t)B * T * s->QP * s->PP;
  return true;
}

// ---- phase A --------------------------------------------------------------------------------------------------------
// Column t of the right-hand side: V0 [B, N, T0] for t < T0, then V1 [B, N, T - T0].
__device__ __forceinline__ float hd_col(const float* V0, int T0, const float* V1, int T1, int64_t b, int64_t N,
                                        int64_t row, int t) {
  return t < T0 ? V0[((size_t)b * N + row) * T0 + t] : V1[((size_t)b * N + row) * T1 + (t - T0)];
}

// grid (S, B, Z); task = t * QT + jt of the WG's TW tasks; wave w: task (w % TW), row pairs kp == w / TW (mod RW).
// acc[it] = C[j = jt*32 + (e&3) + 8(e>>2) + 4h][i = it*32 + (l&31)] = sum_rows v_t G[row, j] F[row, i].
template <int PT>
__global__ __launch_bounds__(kThreads) void k_hd_contract(const float* __restrict__ F, const float* __restrict__ G,
                                                          const float* __restrict__ V0, int T0,
                                                          const float* __restrict__ V1, int T1, int N, int p, int q,
                                                          int QT, int TW, int RW, int chunk, int tasks,
                                                          float* __restrict__ part, const int* __restrict__ stop) {
  if (stop && *stop) return;
  constexpr int PP = 32 * PT;
  constexpr int FS = (PP % 64 == 0) ? PP + 32 : PP;  // row stride of the stage: the two half-waves on other banks
  __shared__ float Fs[kHdKB * FS];
  __shared__ float Gs[kHdKB * 160];
  __shared__ float Vs[kHdKB * 4];
  const int QP = 32 * QT;
  const int GS = (QP % 64 == 0) ? QP + 32 : QP;
  const int T = T0 + T1;
  const int s = blockIdx.x, S = gridDim.x, z = blockIdx.z;
  const int64_t b = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const int task = z * TW + (wave % TW), kq = wave / TW;
  const bool active = task < tasks;
  const int t = active ? task / QT : 0, jt = active ? task % QT : 0;
  const int tlo = (z * TW) / QT;
  const int tl = t - tlo;
  const int thi = min(T - 1, (z * TW + TW - 1) / QT);
  const int r0 = s * chunk, r1 = min(N, r0 + chunk);
  hd_f32x16 acc[PT];
#pragma unroll
  for (int it = 0; it < PT; ++it)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[it][e] = 0.f;
  for (int kr = r0; kr < r1; kr += kHdKB) {
    const int nr = min(kHdKB, r1 - kr);
    __syncthreads();  // (the previous block's products have read the stage)
    for (int e = threadIdx.x; e < kHdKB * PP; e += kThreads) {
      const int r = e / PP, i = e - r * PP;
      Fs[r * FS + i] = (r < nr && i < p) ? F[((size_t)b * N + kr + r) * p + i] : 0.f;
    }
    for (int e = threadIdx.x; e < kHdKB * QP; e += kThreads) {
      const int r = e / QP, j = e - r * QP;
      Gs[r * GS + j] = (r < nr && j < q) ? G[((size_t)b * N + kr + r) * q + j] : 0.f;
    }
    if (threadIdx.x < kHdKB * 4) {
      const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
      Vs[threadIdx.x] = (r < nr && tlo + c <= thi) ? hd_col(V0, T0, V1, T1, b, N, kr + r, tlo + c) : 0.f;
    }
    __syncthreads();
    if (active) {
      for (int kp = kq; kp < kHdKB / 2; kp += RW) {
        const int r = 2 * kp + h;
        const float a = Vs[r * 4 + tl] * Gs[r * GS + jt * 32 + li];
#pragma unroll
        for (int it = 0; it < PT; ++it)
          acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Fs[r * FS + it * 32 + li], acc[it], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  const int slot = s * RW + kq;
  float* out = part + ((((size_t)b * S * RW + slot) * T + t) * QP) * PP;
#pragma unroll
  for (int it = 0; it < PT; ++it)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = jt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      out[(size_t)j * PP + it * 32 + li] = acc[it][e];
    }
}

// M [B, T, QP, PP] = sum_{s < SR} part[B, s, T, QP, PP] in ascending s; Mt [B, T, PP, QP] the transposed copy (optional)
__global__ __launch_bounds__(kThreads) void k_hd_reduce(const float* __restrict__ part, int SR, int64_t per_member,
                                                        int QP, int PP, float* __restrict__ M, float* __restrict__ Mt,
                                                        const int* __restrict__ stop) {
  if (stop && *stop) return;
  const int64_t b = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= per_member) return;
  const float* src = part + (size_t)b * SR * per_member + e;
  float acc = src[0];
  for (int s = 1; s < SR; ++s) acc += src[(size_t)s * per_member];
  M[(size_t)b * per_member + e] = acc;
  if (Mt) {
    const int64_t tq = e / ((int64_t)QP * PP), rem = e - tq * QP * PP;
    const int j = (int)(rem / PP), i = (int)(rem - (int64_t)j * PP);
    Mt[(size_t)b * per_member + (tq * PP + i) * QP + j] = acc;
  }
}

// ---- phases B and C: 64 rows of F and G staged in LDS ---------------------------------------------------------------
// Fs [64][FS2] (FS2 = PP + 1), Gs [64][GS2] (GS2 = QP + 1): odd strides, zero beyond p / q and beyond the last row.
__device__ __forceinline__ void hd_stage_rows(const float* __restrict__ F, const float* __restrict__ G, int64_t b,
                                              int64_t N, int p, int q, int PP, int QP, int64_t row0, int nr, float* Fs,
                                              float* Gs) {
  const int FS2 = PP + 1, GS2 = QP + 1;
  for (int e = threadIdx.x; e < kHdRB * FS2; e += kThreads) {
    const int r = e / FS2, i = e - r * FS2;
    Fs[e] = (r < nr && i < p) ? F[((size_t)b * N + row0 + r) * p + i] : 0.f;
  }
  for (int e = threadIdx.x; e < kHdRB * GS2; e += kThreads) {
    const int r = e / GS2, j = e - r * GS2;
    Gs[e] = (r < nr && j < q) ? G[((size_t)b * N + row0 + r) * q + j] : 0.f;
  }
}

// y[b, row, t] = sum_i F[row, i] (M_t G[row]^T)_i + d o v.  grid (ceil(N / 64), B); tasks (t, it) of a round of kHdTC
// columns over the four waves; acc = C[i = it*32 + (e&3) + 8(e>>2) + 4h][row = l&31 (+32)]; the row-wise dot is summed
// over the registers, then the two half-waves, then the it blocks in LDS (fixed order).
__global__ __launch_bounds__(kThreads) void k_hd_expand(const float* __restrict__ F, const float* __restrict__ G,
                                                        const float* __restrict__ M, const float* __restrict__ dd,
                                                        int dd_mode, const float* __restrict__ v, int N, int p, int q,
                                                        int PT, int QT, int T, float* __restrict__ y,
                                                        const int* __restrict__ stop) {
  if (stop && *stop) return;
  extern __shared__ float sh[];
  const int PP = 32 * PT, QP = 32 * QT, QE = (q + 1) & ~1;
  const int FS2 = PP + 1, GS2 = QP + 1;
  float* Fs = sh;
  float* Gs = Fs + kHdRB * FS2;
  float* ysh = Gs + kHdRB * GS2;  // [kHdTC][PT][64]
  const int64_t b = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * kHdRB;
  const int nr = (int)min((int64_t)kHdRB, N - row0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  hd_stage_rows(F, G, b, N, p, q, PP, QP, row0, nr, Fs, Gs);
  const float* Mb = M + (size_t)b * T * QP * PP;
  for (int t0 = 0; t0 < T; t0 += kHdTC) {
    const int tcn = min(kHdTC, T - t0);
    __syncthreads();  // (stage written / the previous round's sums read)
    for (int task = wave; task < tcn * PT; task += 4) {
      const int tl = task / PT, it = task - tl * PT;
      const float* Mt = Mb + (size_t)(t0 + tl) * QP * PP + it * 32 + li;
      hd_f32x16 a0, a1;
#pragma unroll
      for (int e = 0; e < 16; ++e) a0[e] = a1[e] = 0.f;
      const float* g0 = Gs + li * GS2 + h;
      const float* g1 = Gs + (32 + li) * GS2 + h;
      for (int j0 = 0; j0 < QE; j0 += 2) {
        const float a = Mt[(size_t)(j0 + h) * PP];
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, g0[j0], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, g1[j0], a1, 0, 0, 0);
      }
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int i = it * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        s0 = fmaf(a0[e], Fs[li * FS2 + i], s0);
        s1 = fmaf(a1[e], Fs[(32 + li) * FS2 + i], s1);
      }
      s0 += __shfl_xor(s0, 32, 64);
      s1 += __shfl_xor(s1, 32, 64);
      if (h == 0) {
        ysh[(tl * PT + it) * kHdRB + li] = s0;
        ysh[(tl * PT + it) * kHdRB + 32 + li] = s1;
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nr * tcn; e += kThreads) {
      const int r = e / tcn, tl = e - r * tcn;
      float acc = ysh[tl * PT * kHdRB + r];
      for (int it = 1; it < PT; ++it) acc += ysh[(tl * PT + it) * kHdRB + r];
      const size_t o = ((size_t)b * N + row0 + r) * T + t0 + tl;
      if (dd_mode == LO_DIAG_FULL) acc = fmaf(dd[(size_t)b * N + row0 + r], v[o], acc);
      else if (dd_mode == LO_DIAG_CONST) acc = fmaf(dd[b], v[o], acc);
      y[o] = acc;
    }
  }
}

// dF [B, N, p] and dG [B, N, q] from the contraction M over the 2S columns [v | u] (M^v_t = M_t, M^u_t = M_{S+t}):
//   dF[row, i] = sum_{t < 2S} w_t(row) sum_j M_t[i, j] G[row, j],  dG[row, j] = sum_t w_t(row) sum_i M_t[i, j] F[row, i]
// with w_t = u[:, t] for t < S and v[:, t - S] beyond.  grid (ceil(N / 64), B); tasks: PT blocks of dF then QT of dG.
__global__ __launch_bounds__(kThreads) void k_hd_grad(const float* __restrict__ F, const float* __restrict__ G,
                                                      const float* __restrict__ M, const float* __restrict__ Mtr,
                                                      const float* __restrict__ U, const float* __restrict__ V, int N,
                                                      int p, int q, int PT, int QT, int S, float* __restrict__ dF,
                                                      float* __restrict__ dG) {
  extern __shared__ float sh[];
  const int PP = 32 * PT, QP = 32 * QT, PE = (p + 1) & ~1, QE = (q + 1) & ~1;
  const int FS2 = PP + 1, GS2 = QP + 1;
  float* Fs = sh;
  float* Gs = Fs + kHdRB * FS2;
  const int64_t b = blockIdx.y;
  const int64_t row0 = (int64_t)blockIdx.x * kHdRB;
  const int nr = (int)min((int64_t)kHdRB, N - row0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  hd_stage_rows(F, G, b, N, p, q, PP, QP, row0, nr, Fs, Gs);
  __syncthreads();
  const int T = 2 * S;
  const bool ok0 = li < nr, ok1 = 32 + li < nr;
  const size_t w0 = ((size_t)b * N + row0 + li) * S, w1 = ((size_t)b * N + row0 + 32 + li) * S;
  for (int task = wave; task < PT + QT; task += 4) {
    const bool isF = task < PT;
    const int tile = isF ? task : task - PT;
    // dF: A[i][k = j] = M_t[i, j] from M [T, QP, PP], B[j][row] = w G[row, j];  dG: A[j][k = i] from Mtr [T, PP, QP]
    const float* Ab = isF ? M + (size_t)b * T * QP * PP + tile * 32 + li : Mtr + (size_t)b * T * PP * QP + tile * 32 + li;
    const int lda = isF ? PP : QP;
    const int kext = isF ? QE : PE;
    const float* s0 = isF ? Gs + li * GS2 + h : Fs + li * FS2 + h;
    const float* s1 = isF ? Gs + (32 + li) * GS2 + h : Fs + (32 + li) * FS2 + h;
    const size_t mstride = (size_t)QP * PP;
    hd_f32x16 a0, a1;
#pragma unroll
    for (int e = 0; e < 16; ++e) a0[e] = a1[e] = 0.f;
    for (int t = 0; t < T; ++t) {
      const float* Wsrc = t < S ? U : V;
      const int tc = t < S ? t : t - S;
      const float wt0 = ok0 ? Wsrc[w0 + tc] : 0.f;
      const float wt1 = ok1 ? Wsrc[w1 + tc] : 0.f;
      const float* A = Ab + (size_t)t * mstride;
      for (int k0 = 0; k0 < kext; k0 += 2) {
        const float a = A[(size_t)(k0 + h) * lda];
        a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wt0 * s0[k0], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wt1 * s1[k0], a1, 0, 0, 0);
      }
    }
    float* out = isF ? dF : dG;
    const int width = isF ? p : q;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int c = tile * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (c < width) {
        if (ok0) out[((size_t)b * N + row0 + li) * width + c] = a0[e];
        if (ok1) out[((size_t)b * N + row0 + 32 + li) * width + c] = a1[e];
      }
    }
  }
}

static size_t hd_rows_lds(const HdShape& s, bool with_y) {
  return sizeof(float) * ((size_t)kHdRB * (s.PP + 1) + (size_t)kHdRB * (s.QP + 1) +
                          (with_y ? (size_t)kHdTC * s.PT * kHdRB : 0));
}

// raises the kernel's dynamic LDS limit once to the largest size it takes (p = q = 128)
static int hd_set_lds(const void* fn, bool* done) {
  if (!*done) {
    LO_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    *done = true;
  }
  return LO_OK;
}

// Phase A + reduce: M (and Mt when not null) from the columns [V0 | V1].
static int hd_contract(const HdShape& s, const float* F, const float* G, const float* V0, int T0, const float* V1,
                       float* part, float* M, float* Mt, const int* stop, hipStream_t st) {
  const int T1 = (int)s.T - T0;
  const dim3 grid((unsigned)s.S, (unsigned)s.B, (unsigned)s.Z);
#define HD_CONTRACT(PT_)                                                                                               \
  hipLaunchKernelGGL(k_hd_contract<PT_>, grid, dim3(kThreads), 0, st, F, G, V0, T0, V1, T1, (int)s.N, s.p, s.q, s.QT, \
                     s.TW, s.RW, s.chunk, (int)s.tasks, part, stop)
  LO_PROF_BEGIN("k_hd_contract", st);
  switch (s.PT) {
    case 1: HD_CONTRACT(1); break;
    case 2: HD_CONTRACT(2); break;
    case 3: HD_CONTRACT(3); break;
    default: HD_CONTRACT(4); break;
  }
#undef HD_CONTRACT
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  const int64_t per = s.T * s.QP * s.PP;
  LO_PROF_BEGIN("k_hd_reduce", st);
  hipLaunchKernelGGL(k_hd_reduce, dim3((unsigned)((per + kThreads - 1) / kThreads), (unsigned)s.B), dim3(kThreads), 0,
                     st, part, s.S * s.RW, per, s.QP, s.PP, M, Mt, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

int hadamard_desc_check(const lo_op_desc* op) {
  return (!op->A0 || !op->A1 || op->R < 1 || op->n2 < 1) ? LO_ERR_BADARG : LO_OK;
}

int hadamard_plan(MatvecPlan* pl, Arena* ar, hipStream_t) {
  const lo_op_desc& op = pl->op;
  HdShape s;
  if (const int rc = hadamard_desc_check(&op)) return rc;
  if (!hd_shape(op.B, op.N, op.R, op.n2, pl->c, &s)) return LO_ERR_UNSUPPORTED;
  pl->hd.part = ar->take<float>(s.part_floats);
  pl->hd.m = ar->take<float>(s.m_floats);
  return LO_OK;
}

int hadamard_matvec_run(const MatvecPlan* pl, const float* v, float* y, const int* stop, hipStream_t st) {
  const lo_op_desc& op = pl->op;
  HdShape s;
  if (!hd_shape(op.B, op.N, op.R, op.n2, pl->c, &s)) return LO_ERR_UNSUPPORTED;
  int rc = hd_contract(s, op.A0, op.A1, v, (int)pl->c, nullptr, pl->hd.part, pl->hd.m, nullptr, stop, st);
  if (rc) return rc;
  const size_t lds = hd_rows_lds(s, true);
  static bool lds_set = false;
  if ((rc = hd_set_lds(reinterpret_cast<const void*>(k_hd_expand), &lds_set))) return rc;
  LO_PROF_BEGIN("k_hd_expand", st);
  hipLaunchKernelGGL(k_hd_expand, dim3((unsigned)((s.N + kHdRB - 1) / kHdRB), (unsigned)s.B), dim3(kThreads), lds, st,
                     op.A0, op.A1, pl->hd.m, op.d, op.diag_mode, v, (int)s.N, s.p, s.q, s.PT, s.QT, (int)s.T, y, stop);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

// the workspace of lo_hadamard_bilinear_f32: the contraction partials, M_t of the 2 S columns and its transpose
constexpr size_t kHdBilTail = 512;  // what the sizer reports beyond the layout
struct HdBilBufs { float *part, *M, *Mt; };
static HdBilBufs hd_bil_layout(Arena& ar, const HdShape& s) {  // (a braced list: the takes in this order)
  return {ar.take<float>(s.part_floats), ar.take<float>(s.m_floats), ar.take<float>(s.m_floats)};
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_hadamard_bilinear_workspace_bytes(int64_t B, int64_t N, int64_t p, int64_t q, int64_t S) {
  HdShape s;
  if (!hd_shape(B, N, p, q, 2 * S, &s)) return 0;
  return measured(kHdBilTail, [&](Arena& ar) { hd_bil_layout(ar, s); });
}

int lo_hadamard_bilinear_f32(const float* F, const float* G, const float* U, const float* V, int64_t B, int64_t N,
                             int64_t p, int64_t q, int64_t S, float* dF, float* dG, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!F || !G || !U || !V || !dF || !dG || S < 1) return LO_ERR_BADARG;
  HdShape s;
  if (!hd_shape(B, N, p, q, 2 * S, &s)) return LO_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  Arena ar(ws, ws_bytes, kHdBilTail);
  auto [part, M, Mt] = hd_bil_layout(ar, s);
  if (!ws || !ar.ok) return LO_ERR_WORKSPACE;
  int rc = hd_contract(s, F, G, V, (int)S, U, part, M, Mt, nullptr, st);
  if (rc) return rc;
  const size_t lds = hd_rows_lds(s, false);
  static bool lds_set = false;
  if ((rc = hd_set_lds(reinterpret_cast<const void*>(k_hd_grad), &lds_set))) return rc;
  LO_PROF_BEGIN("k_hd_grad", st);
  hipLaunchKernelGGL(k_hd_grad, dim3((unsigned)((N + kHdRB - 1) / kHdRB), (unsigned)B), dim3(kThreads), lds, st, F, G,
                     M, Mt, U, V, (int)N, s.p, s.q, s.PT, s.QT, (int)S, dF, dG);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

}  // extern "C"
