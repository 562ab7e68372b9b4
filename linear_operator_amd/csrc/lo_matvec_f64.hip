// lo_matvec_f64.hip -- float64 products of the structured operators (ABI 22): lo_matvec_f64 and the two library-side
// callbacks that let lo_cg_solve_f64 / lo_minres_f64 / lo_lanczos_tridiag_f64 run a lowered operator and the Woodbury
// preconditioner without a Python call per product.
//
//   low-rank   y = C (C^T v) + d o v in three plain launches: k64_lr_tn (per-workgroup partials of C^T v over chunks of
//              kLrRows rows), k64_lr_finish (the partials added in chunk order), k64_lr_nn (second pass over C, the
//              [R, c] block and the diagonal in its epilogue).  Loads of C are 16-byte requests along R when R is even
//              and C is 16-byte aligned (two 8-byte loads in the same layout otherwise: the bits do not change).
//              The preconditioner apply z = r / d - Q (Q^T r) | (r - Q Q^T r) / sigma is the same three launches with
//              another epilogue (Epi).
//   dense      k64_dense_mv of lo_cg_f64.hip (f64_dense_mv_ex).
//   Kronecker  two passes of one tiled VALU small-GEMM kernel (k64_kron_gemm), the [n1, n2, c] intermediate in the
//              workspace.  (A v_mfma_f64_16x16x4 variant has not been written)
//   kernel     (ABI 31) LO_OP_KERNEL_DIAG with A0 = X, A1 = theta as doubles: k64_kernel_mv of lo_kernel_op_f64.hip, K never
//              in memory; validated, and its workspace checked, before the first launch of the call.
//   sum        the first term writes y, later terms accumulate into it in their epilogue, the sum's own diagonal goes
//              into the last term's epilogue.
// Every sum runs in a fixed order that depends on the member's own shape only (the row chunks are a function of N, the
// tiles of n1, n2, c): the same inputs give the same bits and a member's result does not depend on the batch around it.
// The kernel kind is the exception to the second half: its column split follows ko_shape(B, M, N), as in
// lo_kernel_mv_f32, so the order of its partial sums depends on B; two calls on the same inputs still give equal bits.
// No float64 atomics.
#include "lo_f64_solver.h"

#include <algorithm>

namespace lo {

constexpr int kLrRows = 256;  // rows of one workgroup's chunk (a constant: the partial sums do not depend on B)
constexpr int kTnCT = 8;      // columns per pass of k64_lr_tn
constexpr int kNnCT = 4;      // columns per pass of k64_lr_nn
constexpr int kNnU = 4;       // row groups a thread of k64_lr_nn carries between two barriers

enum Epi { EPI_OP = 0, EPI_PRE_FULL = 1, EPI_PRE_CONST = 2 };

// Thread layout of the two passes over a tall matrix C [N, R]: RL = R / VEC register slots per row (VEC = 2 for an even
// R: two values per thread), RLc = min(RL, 256) of them side by side, RPP = 256 / RLc rows per pass of the workgroup.
// The layout, and with it the order of every sum, is a function of (N, R) only.  `aligned`: C sits on a 16-byte
// boundary, so a slot of two values is one 16-byte load; otherwise the same slot is read as two 8-byte loads.
struct LrGeom {
  int VEC, RL, RLc, RPP, S, aligned;
};
static LrGeom lr_geom(const double* C, int64_t N, int64_t R) {
  LrGeom g;
  g.VEC = R % 2 == 0 ? 2 : 1;
  g.aligned = ((uintptr_t)C & 15) == 0;
  g.RL = (int)(R / g.VEC);
  g.RLc = std::min(g.RL, kThreads);
  g.RPP = kThreads / g.RLc;
  g.S = (int)((N + kLrRows - 1) / kLrRows);
  return g;
}

template <int VEC>
__device__ __forceinline__ void load_slot(const double* __restrict__ p, int aligned, double (&cv)[VEC]) {
  if constexpr (VEC == 2) {
    if (aligned) {
      const double2 t = *reinterpret_cast<const double2*>(p);
      cv[0] = t.x;
      cv[1] = t.y;
    } else {
      cv[0] = p[0];
      cv[1] = p[1];
    }
  } else {
    cv[0] = p[0];
  }
}

// tpart[b, s, r, j] = sum over the rows i of chunk s of C[b, i, r] v[b, i, j]; grid B * S
template <int VEC>
__global__ __launch_bounds__(kThreads) void k64_lr_tn(const double* __restrict__ C, const double* __restrict__ v,
                                                       double* __restrict__ tpart, int N, int R, int c, int S, int RLc,
                                                       int RPP, int aligned) {
  __shared__ double red[kThreads * VEC * kTnCT];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int row0 = s * kLrRows, row1 = min(N, row0 + kLrRows);
  const int slot = tid % RLc, rowoff = tid / RLc;
  const int RL = R / VEC;
  const double* Cb = C + b * (size_t)N * R;
  const double* vb = v + b * (size_t)N * c;
  double* tp = tpart + (b * S + s) * (size_t)R * c;
  for (int rs0 = 0; rs0 < RL; rs0 += RLc) {
    const int rs = rs0 + slot;
    const bool on = rowoff < RPP && rs < RL;
    for (int j0 = 0; j0 < c; j0 += kTnCT) {
      const int nj = min(kTnCT, c - j0);
      double acc[VEC][kTnCT];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
#pragma unroll
        for (int j = 0; j < kTnCT; ++j) acc[e][j] = 0.0;
      if (on) {
#pragma unroll 2
        for (int i = row0 + rowoff; i < row1; i += RPP) {
          double cv[VEC];
          load_slot<VEC>(Cb + (size_t)i * R + (size_t)rs * VEC, aligned, cv);
          const double* vr = vb + (size_t)i * c + j0;
#pragma unroll
          for (int j = 0; j < kTnCT; ++j)
            if (j < nj) {
              const double x = vr[j];
#pragma unroll
              for (int e = 0; e < VEC; ++e) acc[e][j] += cv[e] * x;
            }
        }
      }
      // the row groups of one slot are added in the order of rowoff
      if (rowoff < RPP) {
        double* mine = red + (size_t)(rowoff * RLc + slot) * (VEC * kTnCT);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
#pragma unroll
          for (int j = 0; j < kTnCT; ++j) mine[e * kTnCT + j] = acc[e][j];
      }
      __syncthreads();
      for (int o = tid; o < RLc * VEC * kTnCT; o += kThreads) {
        const int sl = o / (VEC * kTnCT), rest = o % (VEC * kTnCT);
        const int e = rest / kTnCT, j = rest % kTnCT;
        if (rs0 + sl < RL && j < nj) {
          double t = 0.0;
          for (int ro = 0; ro < RPP; ++ro) t += red[(size_t)(ro * RLc + sl) * (VEC * kTnCT) + rest];
          tp[(size_t)((rs0 + sl) * VEC + e) * c + j0 + j] = t;
        }
      }
      __syncthreads();
    }
  }
}

// t[b, rc] = sum_s tpart[b, s, rc], s ascending
__global__ __launch_bounds__(kThreads) void k64_lr_finish(const double* __restrict__ tpart, double* __restrict__ t,
                                                           int S, int RC, size_t total) {
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const size_t b = e / RC, rc = e % RC;
  const double* p = tpart + b * (size_t)S * RC + rc;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += p[(size_t)s * RC];
  t[e] = acc;
}

// u = C t (slots of a row added in slot order), then per `epi`:
//   EPI_OP         y = [y +] u + d o v
//   EPI_PRE_FULL   y = v / d - u          EPI_PRE_CONST   y = (v - u) / d[b]
template <int VEC>
__global__ __launch_bounds__(kThreads) void k64_lr_nn(const double* __restrict__ C, const double* __restrict__ t,
                                                       const double* __restrict__ dd, int dmode,
                                                       const double* __restrict__ v, double* __restrict__ y, int N,
                                                       int R, int c, int S, int RLc, int RPP, int epi, int accumulate,
                                                       int aligned) {
  __shared__ double red[kNnU * kThreads * kNnCT];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int row0 = s * kLrRows, row1 = min(N, row0 + kLrRows);
  const int slot = tid % RLc, rowoff = tid / RLc;
  const int RL = R / VEC;
  const bool single = RL <= RLc;  // every slot of a row sits in one thread group: its part of t stays in registers
  const double* Cb = C + b * (size_t)N * R;
  const double* tb = t + b * (size_t)R * c;
  const double* vb = v + b * (size_t)N * c;
  double* yb = y + b * (size_t)N * c;
  for (int j0 = 0; j0 < c; j0 += kNnCT) {
    const int nj = min(kNnCT, c - j0);
    double tv[VEC][kNnCT];
#pragma unroll
    for (int e = 0; e < VEC; ++e)
#pragma unroll
      for (int j = 0; j < kNnCT; ++j)
        tv[e][j] = (single && slot < RL && j < nj) ? tb[(size_t)(slot * VEC + e) * c + j0 + j] : 0.0;
    for (int ibase = row0; ibase < row1; ibase += RPP * kNnU) {
      if (rowoff < RPP) {
#pragma unroll
        for (int u = 0; u < kNnU; ++u) {
          const int i = ibase + u * RPP + rowoff;
          double p[kNnCT];
#pragma unroll
          for (int j = 0; j < kNnCT; ++j) p[j] = 0.0;
          if (i < row1) {
            for (int rs0 = 0; rs0 < RL; rs0 += RLc) {
              const int rs = rs0 + slot;
              if (rs < RL) {
                double cv[VEC];
                load_slot<VEC>(Cb + (size_t)i * R + (size_t)rs * VEC, aligned, cv);
#pragma unroll
                for (int e = 0; e < VEC; ++e)
#pragma unroll
                  for (int j = 0; j < kNnCT; ++j) {
                    const double tt = single ? tv[e][j] : (j < nj ? tb[(size_t)(rs * VEC + e) * c + j0 + j] : 0.0);
                    p[j] += cv[e] * tt;
                  }
              }
            }
          }
#pragma unroll
          for (int j = 0; j < kNnCT; ++j) red[(size_t)((u * RPP + rowoff) * kNnCT + j) * RLc + slot] = p[j];
        }
      }
      __syncthreads();
      for (int o = tid; o < RPP * kNnU * nj; o += kThreads) {
        const int rr = o / nj, j = o % nj;
        const int i = ibase + rr;
        if (i < row1) {
          const double* q = red + (size_t)(rr * kNnCT + j) * RLc;
          double r = 0.0;
          for (int sl = 0; sl < RLc; ++sl) r += q[sl];
          const size_t off = (size_t)i * c + j0 + j;
          const double x = vb[off];
          if (epi == EPI_OP) {
            if (accumulate) r = yb[off] + r;
            if (dmode == LO_DIAG_FULL) r += dd[b * N + i] * x;
            if (dmode == LO_DIAG_CONST) r += dd[b] * x;
          } else if (epi == EPI_PRE_FULL) {
            r = x / dd[b * N + i] - r;
          } else {
            r = (x - r) / dd[b];
          }
          yb[off] = r;
        }
      }
      __syncthreads();
    }
  }
}

// Small GEMM with strided operands, one member per blockIdx.z, a 32 x 32 tile of outputs per workgroup, k ascending:
//   out[b][m osm + q1 osq1 + q2] = sum_k A[b][m Kd + k] X[b][k xsk + q1 xsq1 + q2],   q = q1 Q2 + q2 < Q1 Q2
// epi_on (second Kronecker pass, out = y at offset row * c + column): out = [out +] sum + d o v.
constexpr int kGT = 32, kGK = 16;
struct KronGemm {
  const double* A;
  const double* X;
  double* out;
  size_t a_sb, x_sb, o_sb;
  int M, Kd, Q1, Q2;
  long long xsk, xsq1, osm, osq1;
  int kfast, mfast;  // consecutive threads along k when loading X / along m when storing (the contiguous direction)
  int epi_on, dmode, accumulate, c, N;
  const double* dd;
  const double* v;
};
__global__ __launch_bounds__(kThreads) void k64_kron_gemm(KronGemm g) {
  __shared__ double As[kGK][kGT + 1];
  __shared__ double Xs[kGK][kGT + 1];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.z;
  const int m0 = blockIdx.y * kGT, q0 = blockIdx.x * kGT;
  const long long Q = (long long)g.Q1 * g.Q2;
  const int tm = g.mfast ? tid % 16 : tid / 16;
  const int tq = g.mfast ? tid / 16 : tid % 16;
  const double* Ab = g.A + b * g.a_sb;
  const double* Xb = g.X + b * g.x_sb;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int k0 = 0; k0 < g.Kd; k0 += kGK) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = tid + kThreads * u;
      {
        const int kk = e % kGK, mm = e / kGK;
        const int m = m0 + mm, k = k0 + kk;
        As[kk][mm] = (m < g.M && k < g.Kd) ? Ab[(size_t)m * g.Kd + k] : 0.0;
      }
      {
        const int kk = g.kfast ? e % kGK : e / kGT;
        const int qq = g.kfast ? e / kGK : e % kGT;
        const long long q = q0 + qq;
        const int k = k0 + kk;
        double x = 0.0;
        if (k < g.Kd && q < Q) x = Xb[(size_t)(k * g.xsk + (q / g.Q2) * g.xsq1 + (q % g.Q2))];
        Xs[kk][qq] = x;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGK; ++kk) {
      const double a0 = As[kk][tm], a1 = As[kk][tm + 16];
      const double x0 = Xs[kk][tq], x1 = Xs[kk][tq + 16];
      acc[0][0] += a0 * x0;
      acc[0][1] += a0 * x1;
      acc[1][0] += a1 * x0;
      acc[1][1] += a1 * x1;
    }
    __syncthreads();
  }
  double* ob = g.out + b * g.o_sb;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      const int m = m0 + tm + 16 * a;
      const long long q = q0 + tq + 16 * w;
      if (m >= g.M || q >= Q) continue;
      const size_t off = (size_t)(m * g.osm + (q / g.Q2) * g.osq1 + (q % g.Q2));
      double r = acc[a][w];
      if (g.epi_on) {
        if (g.accumulate) r = ob[off] + r;
        if (g.dmode != LO_DIAG_NONE) {
          const double x = g.v[b * (size_t)g.N * g.c + off];
          r += (g.dmode == LO_DIAG_FULL ? g.dd[b * (size_t)g.N + off / g.c] : g.dd[b]) * x;
        }
      }
      ob[off] = r;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static bool lr_shape_ok(int64_t B, int64_t N, int64_t R, int64_t c) {
  const int64_t S = (N + kLrRows - 1) / kLrRows;
  return B >= 1 && N >= 1 && R >= 1 && c >= 1 && N <= 0x7ffffff0 && R <= 0x7fffffff / 2 && c <= 0x7fffffff / 2 &&
         B * S <= 0x7fffffff && R * c <= 0x7fffffff;
}

static void lr_layout(int64_t B, int64_t N, int64_t R, int64_t c, Arena& ar, double** tpart, double** t) {
  const size_t S = (size_t)((N + kLrRows - 1) / kLrRows);
  *tpart = ar.take<double>((size_t)B * S * R * c);
  *t = ar.take<double>((size_t)B * R * c);
}

// y = epilogue(C (C^T v)) for a tall C [B, N, R]: the operator's product and the preconditioner apply
static int lr_run(const double* C, int64_t B, int64_t N, int64_t R, int64_t c, const double* dd, int dmode, int epi,
                  int accumulate, const double* v, double* y, Arena& ar, hipStream_t st) {
  if (!lr_shape_ok(B, N, R, c)) return LO_ERR_UNSUPPORTED;
  double *tpart, *t;
  lr_layout(B, N, R, c, ar, &tpart, &t);
  if (!ar.ok) return LO_ERR_WORKSPACE;
  const LrGeom g = lr_geom(C, N, R);
  const dim3 grid((unsigned)(B * g.S));
  const size_t total = (size_t)B * R * c;
  if (g.VEC == 2)
    hipLaunchKernelGGL(k64_lr_tn<2>, grid, dim3(kThreads), 0, st, C, v, tpart, (int)N, (int)R, (int)c, g.S, g.RLc, g.RPP,
                       g.aligned);
  else
    hipLaunchKernelGGL(k64_lr_tn<1>, grid, dim3(kThreads), 0, st, C, v, tpart, (int)N, (int)R, (int)c, g.S, g.RLc, g.RPP,
                       g.aligned);
  LO_LAUNCH_CHECK();
  hipLaunchKernelGGL(k64_lr_finish, elem_grid(total), dim3(kThreads), 0, st, tpart, t, g.S, (int)(R * c), total);
  LO_LAUNCH_CHECK();
  if (g.VEC == 2)
    hipLaunchKernelGGL(k64_lr_nn<2>, grid, dim3(kThreads), 0, st, C, t, dd, dmode, v, y, (int)N, (int)R, (int)c, g.S,
                       g.RLc, g.RPP, epi, accumulate, g.aligned);
  else
    hipLaunchKernelGGL(k64_lr_nn<1>, grid, dim3(kThreads), 0, st, C, t, dd, dmode, v, y, (int)N, (int)R, (int)c, g.S,
                       g.RLc, g.RPP, epi, accumulate, g.aligned);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

static bool kron_shape_ok(int64_t B, int64_t n1, int64_t n2, int64_t c) {
  return B >= 1 && B <= 65535 && n1 >= 1 && n2 >= 1 && c >= 1 && n1 * n2 <= 0x7ffffff0 && n1 * c <= 0x7ffffff0 &&
         n2 * c <= 0x7ffffff0 && (n1 + kGT - 1) / kGT <= 65535 && (n2 + kGT - 1) / kGT <= 65535;
}

static double* kron_layout(int64_t B, int64_t N, int64_t c, Arena& ar) { return ar.take<double>((size_t)B * N * c); }

static int kron_run(const double* K1, const double* K2, int64_t B, int64_t n1, int64_t n2, int64_t c, const double* dd,
                    int dmode, int accumulate, const double* v, double* y, Arena& ar, hipStream_t st) {
  if (!kron_shape_ok(B, n1, n2, c)) return LO_ERR_UNSUPPORTED;
  const int64_t N = n1 * n2;
  double* tmp = kron_layout(B, N, c, ar);
  if (!ar.ok) return LO_ERR_WORKSPACE;
  KronGemm a{};  // tmp[i1, k2, j] = sum_i2 K2[k2, i2] v[i1, i2, j]
  a.A = K2, a.X = v, a.out = tmp;
  a.a_sb = (size_t)n2 * n2, a.x_sb = a.o_sb = (size_t)N * c;
  a.M = (int)n2, a.Kd = (int)n2, a.Q1 = (int)n1, a.Q2 = (int)c;
  a.xsk = c, a.xsq1 = n2 * c, a.osm = c, a.osq1 = n2 * c;
  a.kfast = a.mfast = c < 8;
  a.c = (int)c, a.N = (int)N;
  hipLaunchKernelGGL(k64_kron_gemm, dim3((unsigned)((n1 * c + kGT - 1) / kGT), (unsigned)((n2 + kGT - 1) / kGT), (unsigned)B),
                     dim3(kThreads), 0, st, a);
  LO_LAUNCH_CHECK();
  KronGemm p{};  // y[k1, k2, j] = sum_i1 K1[k1, i1] tmp[i1, k2, j]
  p.A = K1, p.X = tmp, p.out = y;
  p.a_sb = (size_t)n1 * n1, p.x_sb = p.o_sb = (size_t)N * c;
  p.M = (int)n1, p.Kd = (int)n1, p.Q1 = 1, p.Q2 = (int)(n2 * c);
  p.xsk = n2 * c, p.xsq1 = 0, p.osm = n2 * c, p.osq1 = 0;
  p.epi_on = 1, p.dmode = dmode, p.accumulate = accumulate, p.c = (int)c, p.N = (int)N, p.dd = dd, p.v = v;
  hipLaunchKernelGGL(k64_kron_gemm, dim3((unsigned)((n2 * c + kGT - 1) / kGT), (unsigned)((n1 + kGT - 1) / kGT), (unsigned)B),
                     dim3(kThreads), 0, st, p);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

static bool plain_kind(int kind) {
  return kind == LO_OP_LOWRANK_DIAG || kind == LO_OP_DENSE_DIAG || kind == LO_OP_KRON_DIAG || kind == LO_OP_KERNEL_DIAG;
}

constexpr size_t kMv64Tail = 1024, kPre64Tail = 1024;  // what the matvec / preconditioner sizer reports behind its layout

// What term_run takes for one term, through the layout function of the term's kind: nothing for the dense kind, for a
// kind lo_matvec_f64 refuses and for a kernel term its check refuses.
static void term_layout(const lo_op_desc* op, int64_t c, Arena& ar) {
  if (op->kind == LO_OP_LOWRANK_DIAG) {
    double *a, *b;
    lr_layout(op->B, op->N, op->R, c, ar, &a, &b);
  } else if (op->kind == LO_OP_KRON_DIAG) {
    kron_layout(op->B, op->N, c, ar);
  } else if (op->kind == LO_OP_KERNEL_DIAG) {
    if (kernel_desc_check_f64(op, c) == LO_OK) kernel_mv_layout_f64(ar, op->B, op->N, op->N, c);
  }
}

static int term_run(const lo_op_desc* op, const double* dd, int dmode, int accumulate, const double* v, double* y,
                    int64_t c, Arena& ar, hipStream_t st) {
  const double* A0 = (const double*)op->A0;
  if (!A0) return LO_ERR_BADARG;
  switch (op->kind) {
    case LO_OP_LOWRANK_DIAG:
      return lr_run(A0, op->B, op->N, op->R, c, dd, dmode, EPI_OP, accumulate, v, y, ar, st);
    case LO_OP_DENSE_DIAG:
      if (op->B > 65535 || op->N > 0x7ffffff0 || c > 0x7fffffff / 2) return LO_ERR_UNSUPPORTED;
      return f64_dense_mv_ex(A0, dd, dmode, accumulate, v, y, op->B, op->N, c, st);
    case LO_OP_KRON_DIAG:
      if (!op->A1 || op->R < 1 || op->n2 < 1 || op->R * op->n2 != op->N) return LO_ERR_BADARG;
      return kron_run(A0, (const double*)op->A1, op->B, op->R, op->n2, c, dd, dmode, accumulate, v, y, ar, st);
    case LO_OP_KERNEL_DIAG: {  // (checked by the caller before the first launch: kernel_terms_check)
      double* part = kernel_mv_layout_f64(ar, op->B, op->N, op->N, c);
      if (!ar.ok) return LO_ERR_WORKSPACE;
      return kernel_mv_run_f64(A0, A0, (const double*)op->A1, (int)op->n2, op->B, op->N, op->N, op->R, v, c, dd, dmode,
                               accumulate, y, part, st);
    }
    default:
      return LO_ERR_UNSUPPORTED;
  }
}

// a kernel term is validated, and its workspace measured against what the caller gave, before anything is launched
static int kernel_term_check(const lo_op_desc* op, int64_t c, size_t ws_bytes, const void* ws) {
  if (op->kind != LO_OP_KERNEL_DIAG) return LO_OK;
  const int rc = kernel_desc_check_f64(op, c);
  if (rc) return rc;
  const size_t need = measured(0, [&](Arena& ar) { term_layout(op, c, ar); });
  return (need > ws_bytes || (need && !ws)) ? LO_ERR_WORKSPACE : LO_OK;
}

static int diag_ok(const lo_op_desc* op) {
  if (op->diag_mode == LO_DIAG_NONE) return 1;
  return (op->diag_mode == LO_DIAG_FULL || op->diag_mode == LO_DIAG_CONST) && op->d != nullptr;
}

}  // namespace lo

using namespace lo;

extern "C" size_t lo_matvec_f64_workspace_bytes(const lo_op_desc* op, int64_t c) {
  if (!op || c < 1 || op->B < 1 || op->N < 1) return 0;
  if (op->kind != LO_OP_SUM) return measured(kMv64Tail, [&](Arena& ar) { term_layout(op, c, ar); });
  if (!op->terms || op->nterms < 2 || op->nterms > LO_MAX_TERMS) return 0;
  return measured(kMv64Tail, [&](Arena& ar) {  // (the terms share the workspace: the largest of them)
    for (int i = 0; i < op->nterms; ++i) {
      Arena term(nullptr, 0);
      term_layout(&op->terms[i], c, term);
      ar.off = std::max(ar.off, term.off);
    }
  });
}

extern "C" int lo_matvec_f64(const lo_op_desc* op, const double* v, double* y, int64_t c, void* ws, size_t ws_bytes,
                             void* stream) {
  if (!op || !v || !y || v == y) return LO_ERR_BADARG;
  if (op->kind != LO_OP_SUM && !plain_kind(op->kind)) return LO_ERR_UNSUPPORTED;
  if (op->B < 1 || op->N < 1 || c < 1 || !diag_ok(op)) return LO_ERR_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const double* dd = (const double*)op->d;
  if (op->kind != LO_OP_SUM) {
    if (const int rc = kernel_term_check(op, c, ws_bytes, ws)) return rc;
    Arena ar(ws, ws_bytes);
    return term_run(op, dd, op->diag_mode, 0, v, y, c, ar, st);
  }
  if (!op->terms || op->nterms < 2 || op->nterms > LO_MAX_TERMS) return LO_ERR_BADARG;
  for (int i = 0; i < op->nterms; ++i) {
    const lo_op_desc* t = &op->terms[i];
    if (!plain_kind(t->kind)) return LO_ERR_UNSUPPORTED;
    if (t->diag_mode != LO_DIAG_NONE || t->B != op->B || t->N != op->N) return LO_ERR_BADARG;
    if (const int rc = kernel_term_check(t, c, ws_bytes, ws)) return rc;
  }
  for (int i = 0; i < op->nterms; ++i) {
    const bool last = i == op->nterms - 1;
    Arena ar(ws, ws_bytes);  // (the terms run one after the other on `stream`: they share the workspace)
    const int rc = term_run(&op->terms[i], last ? dd : nullptr, last ? op->diag_mode : LO_DIAG_NONE, i > 0, v, y, c, ar, st);
    if (rc) return rc;
  }
  return LO_OK;
}

extern "C" int lo_matvec_desc_cb_f64(void* user, const double* v, double* y, int64_t B, int64_t N, int64_t c,
                                     void* stream) {
  const lo_f64_op_ctx* ctx = (const lo_f64_op_ctx*)user;
  if (!ctx || !ctx->op || ctx->op->B != B || ctx->op->N != N) return LO_ERR_BADARG;
  return lo_matvec_f64(ctx->op, v, y, c, ctx->ws, ctx->ws_bytes, stream);
}

extern "C" size_t lo_precond_f64_workspace_bytes(int64_t B, int64_t N, int32_t k, int64_t c) {
  if (B < 1 || N < 1 || k < 1 || c < 1) return 0;
  double *a, *b;
  return measured(kPre64Tail, [&](Arena& ar) { lr_layout(B, N, k, c, ar, &a, &b); });
}

extern "C" int lo_precond_desc_cb_f64(void* user, const double* r, double* z, int64_t B, int64_t N, int64_t c,
                                      void* stream) {
  const lo_f64_precond_ctx* ctx = (const lo_f64_precond_ctx*)user;
  if (!ctx || !ctx->Q || !ctx->noise || !r || !z || r == z || ctx->k < 1) return LO_ERR_BADARG;
  if (ctx->diag_mode != LO_DIAG_FULL && ctx->diag_mode != LO_DIAG_CONST) return LO_ERR_BADARG;
  Arena ar(ctx->ws, ctx->ws_bytes);
  return lr_run(ctx->Q, B, N, ctx->k, c, ctx->noise, ctx->diag_mode,
                ctx->diag_mode == LO_DIAG_FULL ? EPI_PRE_FULL : EPI_PRE_CONST, 0, r, z, ar, (hipStream_t)stream);
}
