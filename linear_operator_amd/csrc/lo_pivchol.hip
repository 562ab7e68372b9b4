// lo_pivchol.hip -- greedy partial pivoted Cholesky, restating PivotedCholesky.forward
// (linear_operator/functions/_pivoted_cholesky.py:14-105) with the row fetch
// (utils/permutation.py:9-88 -> LinearOperator.__getitem__ -> operator _get_indices) generated on the fly
// from the operator descriptor.  One line per kind: entry (p, i) of the row of pivot p, the diagonal, the reference's
// lines where it has the operator, and the functions that hold the formula (every kind's diagonal is a branch of
// src_diag, its row a branch of src_entry, its descriptor check a case of pc_check_desc):
//   LOWRANK        sum_r C[p,r] C[i,r]; diag sum_r C[i,r]^2 (root_linear_operator.py:37-50, :22-28)
//                  -- seq_dot over the LDS tile of stage_rows, in k_pc_init / k_pc_update themselves
//   DENSE          K[p,i]; diag K[i,i] (dense_linear_operator.py:47-50, :37-40)
//   KRON           K1[p1,i1] K2[p2,i2]; diag K1[i1,i1] K2[i2,i2] (kronecker_product_linear_operator.py:198-216, :22-28)
//   CALLBACK       the row and the diagonal the caller's callback fetched (LinearOperator.__getitem__ / _diagonal)
//   SUM            the terms' rows / diagonals added left to right (sum_linear_operator.py:31-45) -- the term loops
//                  of k_pc_init / k_pc_update
//   HADAMARD       (F_p . F_i)(G_p . G_i); diag |F_i|^2 |G_i|^2 (mul_linear_operator.py:49-52, :43-47) -- seq_dot
//   TOEPLITZ       t[|p - i|]; diag t[0] (toeplitz_linear_operator.py:38-40, :25-31)
//   TOEPLITZ_KRON  prod_k t_k[|p_k - i_k|], leading factor first; diag prod_k t_k[0], trailing factors first
//                  (kronecker_product_linear_operator.py:198-216, :22-28 over the Toeplitz rows) -- grid_base, grid_t0
//   SKI            sum_b sum_a t[|li[p,a] - ri[i,b]|] (lv[p,a] rv[i,b]) (interpolated_linear_operator.py:130-144);
//                  diag the reference's APPROXIMATE one, (W_l sqrt t0) o (W_r sqrt t0), t0 = t[0] (:94-101,
//                  functions/_pivoted_cholesky.py:25): pivots are chosen on it, rows come from the true matrix
//                  -- ski_entry<T, false>, ski_approx_diag
//   SKI_GRID       the same with t[|.|] replaced by the TOEPLITZ_KRON entry of the grid points and t0 = prod_k t_k[0]
//                  -- ski_entry<T, true> over grid_base, ski_approx_diag over grid_t0
//   SKI_SUM        sum over the terms of the SKI entry, terms ascending (sum_batch_linear_operator.py:43-52); diag
//                  the EXACT one, entry (i, i) of the same sum (SumBatch has no approximate diagonal: _approx_diagonal
//                  is _diagonal, :37-41) -- ski_entry<T, false> in both
//   KERNEL         os2 g(r2), r2 = |theta o x_p - theta o x_i|^2 summed over the coordinates in ascending order; diag
//                  os2 (kernel_linear_operator.py:230-246, :263-279) -- kern_r2, kf_g_rt (lo_kernel_fn.h)
//   KERNEL_SUM     sum_t os2_t g_t(r2_t), terms ascending; diag sum_t os2_t (sum_linear_operator.py:31-45 over
//                  KERNEL terms on one point tensor) -- kern_r2 per term
//   KERNEL_KRON    (os2 g(r2_pj)) Bt[tau, s] for p = (p, tau), i = (j, s); diag os2 Bt[tau, tau]
//                  (kronecker_product_linear_operator.py:198-216 over KERNEL and the task matrix) -- kern_r2
//   KERNEL_LMC     sum_q (os2_q g_q(r2_q,pj)) B_q[tau, s], terms ascending; diag sum_q os2_q B_q[tau, tau]
//                  (sum_linear_operator.py:31-45 over KERNEL_KRON terms on one point tensor) -- kern_r2 per term
//   KERNEL_TASK    (os2 g(r2_pi)) Bt[t_p, t_i], the task ids in the points' last column; diag os2 Bt[t_i, t_i]
//                  (no operator of the reference: include/lo_amd.h, LO_OP_KERNEL_TASK_DIAG) -- kern_r2, tk_task_id
//   KERNEL_PARAM   os2 g(x_p, x_i), g rational quadratic or periodic; diag os2 (no operator of the reference: include/lo_amd.h,
//                  LO_OP_KERNEL_PARAM_DIAG) -- kp_g_rt (lo_kernel_fn.h)
//   KERNEL_SM      sum_q w_q E_q prod_k cos(2 pi mu_qk tau_k), the spectral mixture; diag sum_q w_q in ascending q (no operator of
//                  the reference: include/lo_amd.h, LO_OP_KERNEL_SM_DIAG) -- ksm_g_rt (lo_kernel_fn.h)
//   KERNEL_GRAD    the (al, be) entry of the RBF value / derivative block of the points p, j; diag os2, os2 t_a^2
//                  (no operator of the reference: include/lo_amd.h, lo_kernel_grad_mv_f32) -- its own loop: that of
//                  kern_r2, which also keeps the scaled differences of the coordinates al, be
// Integer results (pivots, permutation) must match the CPU path bit for bit, so every value that feeds
// a pivot decision is computed per element in a FIXED order with individually rounded operations
// (products rounded before summation, sequential in r and in j; this file is compiled with
// -ffp-contract=off AND carries the pragma below, because HIP's __fmul_rn/__fadd_rn are plain * and +
// that hipcc's default fp-contract=fast would fuse, and __fsqrt_rn is the 1-ulp native sqrt; sqrtf and /
// are correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt) -- the same
// order oracle/lo_oracle.py uses.  Batch-global control flow (one shared rank
// m, loop while max_b error > tol, :57) is decided on the device by a single-workgroup control kernel;
// the host enqueues all max_rank pivots and reads m back once.
//
// HBM traffic per pivot m and member: row source (C: 4NR B; dense: 4N; kron: ~0) + 4 m N (L rows 0..m-1)
// + ~24 N (diag, perm, L row m).
#include <algorithm>
#pragma clang fp contract(off)

#include "lo_device.h"
#include <string.h>

#include "lo_internal.h"
#include "lo_kernel_fn.h"
#include "lo_kernel_task.h"

namespace lo {

struct PcCtrl {
  int stop;
  int m;  // pivots taken so far
};

template <typename T>
struct PcDevT {
  lo_op_desc op;
  // the terms whose rows / diagonals are summed left to right (SumLinearOperator._diagonal / _getitem of the
  // reference, sum_linear_operator.py:31-45): one entry for a plain operator
  int nterms;
  lo_op_desc terms[LO_MAX_TERMS];
  lo_interp_desc ski;  // LO_OP_SKI_DIAG: the interpolation matrices (a device-side copy of the host struct op.interp);
                       // LO_OP_TOEPLITZ_KRON_DIAG: only grid_ndim / grid_m, copied from the host struct op.grid
  int64_t B, N;
  int S, rows;     // position split
  int max_rank;
  T tol;
  T* diag;       // [B,N]
  T* L;          // [B,max_rank,N]
  long long* perm;   // [B,N]
  long long* pim;    // [B]
  T* maxval;     // [B]
  T* part_a;     // [B,S]  (max / error partials)
  T* part_b;     // [B,S]
  T* orig;       // [B]
  T* errors;     // [B]
  T* arg_v;      // [B,S] per-slice argmax partial (value)
  int* arg_j;        // [B,S]                          (position)
  PcCtrl* ctrl;
};

// scalar-type helpers of the templated engine (float: the hot path; double: the reference is dtype-generic,
// functions/_pivoted_cholesky.py:14-105 -- same operation order, so pivots agree with a float64 run of the reference)
template <typename T> __device__ __forceinline__ T pc_sqrt(T x);
template <> __device__ __forceinline__ float pc_sqrt<float>(float x) { return sqrtf(x); }
template <> __device__ __forceinline__ double pc_sqrt<double>(double x) { return sqrt(x); }
template <typename T> __device__ __forceinline__ T pc_abs(T x) { return x < T(0) ? -x : x; }
template <typename T> __device__ __forceinline__ T pc_max(T a, T b) { return (a != a) ? b : ((b != b) ? a : (a > b ? a : b)); }
template <typename T> __device__ __forceinline__ T pc_ninf() { return -(T)INFINITY; }
template <typename T> __device__ __forceinline__ const T* pc_ptr(const float* p) { return reinterpret_cast<const T*>(p); }
// block reductions over 256 threads through `red` (256 elements of T): fixed tree order, result in every thread
__device__ __forceinline__ float pc_block_sum(float v, float* red) { return block_sum256(v, red); }  // (round 1-3 order)
__device__ __forceinline__ float pc_block_max(float v, float* red) { return block_max256(v, red); }
template <typename T, typename Op>
__device__ __forceinline__ T pc_block_reduce(T v, T* red, Op op) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + h]);
    __syncthreads();
  }
  return red[0];
}
template <typename T>
__device__ __forceinline__ T pc_block_sum(T v, T* red) { return pc_block_reduce(v, red, [](T a, T b) { return a + b; }); }
template <typename T>
__device__ __forceinline__ T pc_block_max(T v, T* red) { return pc_block_reduce(v, red, [](T a, T b) { return pc_max(a, b); }); }

template <typename T>
__device__ __forceinline__ T seq_dot(const T* __restrict__ a, const T* __restrict__ b, int R) {
  // acc = a0*b0; acc = acc + a_r*b_r  (sequential, product rounded first)
  T acc = a[0] * b[0];
  for (int r = 1; r < R; ++r) acc = acc + a[r] * b[r];
  return acc;
}

// ---- the pieces the row sources share, each formula once ------------------------------------------------------------
// |theta o (x_p - x_i)|^2 of two points of D coordinates: the coordinates scaled and rounded separately, then
// differenced, the squares summed in ascending k
__device__ __forceinline__ float kern_r2(const float* xp, const float* xi, const float* th, int D) {
  float r2 = 0.0f;
  for (int k = 0; k < D; ++k) {
    const float df = xp[k] * th[k] - xi[k] * th[k];
    r2 = r2 + df * df;
  }
  return r2;
}

// the first columns of member b of a Kronecker product of D = 2 / 3 Toeplitz factors (shape: d.ski.grid_*): the two
// trailing axes c1, c2 and, D == 3, the leading one c0
template <typename T>
struct GridCols { int D, m1, m2; const T *c0, *c1, *c2; };
template <typename T>
__device__ __forceinline__ GridCols<T> grid_cols(const PcDevT<T>& d, const float* A0, int64_t b) {
  const int D = d.ski.grid_ndim, m0 = D == 3 ? (int)d.ski.grid_m[0] : 0;
  const int m1 = (int)d.ski.grid_m[D - 2], m2 = (int)d.ski.grid_m[D - 1];
  const T* c0 = pc_ptr<T>(A0) + (size_t)b * (m0 + m1 + m2);
  return {D, m1, m2, c0, c0 + m0, c0 + m0 + m1};
}
struct GridPt { int k0, k1, k2; };  // the coordinates of grid point k0 (m1 m2) + k1 m2 + k2
template <typename T>
__device__ __forceinline__ GridPt grid_pt(const GridCols<T>& g, int p) {
  return {p / (g.m2 * g.m1), (p / g.m2) % g.m1, p % g.m2};
}
// prod_k t_k[|p_k - q_k|] of the grid points p and q, the leading factor multiplied first; consecutive threads hold
// consecutive positions: the gathers from the (small) columns stay in cache
template <typename T>
__device__ __forceinline__ T grid_base(const GridCols<T>& g, const GridPt& p, const GridPt& q) {
  const T f1 = g.c1[p.k1 > q.k1 ? p.k1 - q.k1 : q.k1 - p.k1], f2 = g.c2[p.k2 > q.k2 ? p.k2 - q.k2 : q.k2 - p.k2];
  return g.D == 3 ? (g.c0[p.k0 > q.k0 ? p.k0 - q.k0 : q.k0 - p.k0] * f1) * f2 : f1 * f2;
}
// its constant diagonal prod_k t_k[0], the trailing factors multiplied first
template <typename T>
__device__ __forceinline__ T grid_t0(const GridCols<T>& g) {
  const T t0 = g.c1[0] * g.c2[0];
  return g.D == 3 ? g.c0[0] * t0 : t0;
}

// entry (pim, i) of W_l K W_r^T of term tm, member g of its interpolation arrays and columns: base[p, q] *
// (lv[pim, a] rv[i, b']) summed over both, b' outside (interpolated_linear_operator.py:139-144).  base[p, q] is
// t[|p - q|] of the member's column, or (GRID) grid_base; a grid point outside [0, M) contributes T(0) and reads nothing
template <typename T, bool GRID>
__device__ __forceinline__ T ski_entry(const PcDevT<T>& d, const lo_op_desc& tm, size_t g, int pim, int i) {
  // (N <= 0x7ffffff0 by pc_check_desc: read as the kernels' 32-bit N; GRID: M <= LO_SKI_GRID_MAX_M, 32-bit grid points)
  const int64_t M = tm.R, N = (int)d.N;
  const int J = (int)tm.n2;
  const T* col = GRID ? nullptr : pc_ptr<T>(tm.A0) + g * M;  // 1-D: the member's first column
  GridCols<T> gc{};
  if constexpr (GRID) gc = grid_cols(d, tm.A0, (int64_t)g);
  const int64_t* li = d.ski.left_idx + (g * N + pim) * J;
  const T* lv = pc_ptr<T>(d.ski.left_vals) + (g * N + pim) * J;
  const int64_t* ri = d.ski.right_idx + (g * N + i) * J;
  const T* rv = pc_ptr<T>(d.ski.right_vals) + (g * N + i) * J;
  T tv = T(0);
  for (int bb = 0; bb < J; ++bb) {
    const int64_t q = ri[bb];
    const bool q_in = q >= 0 && q < M;
    GridPt qq{};
    if constexpr (GRID) qq = grid_pt(gc, q_in ? (int)q : 0);  // (once per b')
    for (int a = 0; a < J; ++a) {
      const int64_t p = li[a];
      const bool in = p >= 0 && p < M && q_in;
      T bv = T(0);
      if constexpr (GRID) {
        if (in) bv = grid_base(gc, grid_pt(gc, (int)p), qq);
      } else {
        if (in) bv = col[p > q ? p - q : q - p];
      }
      tv = (bb == 0 && a == 0) ? bv * (lv[a] * rv[bb]) : tv + bv * (lv[a] * rv[bb]);
    }
  }
  return tv;
}
// the reference's approximate SKI diagonal over a constant base diagonal t0 = s^2:
// left_interp(li, lv, s) * left_interp(ri, rv, s) at row i
template <typename T>
__device__ __forceinline__ T ski_approx_diag(const lo_interp_desc& w, int64_t M, int J, size_t row, T s) {
  const int64_t *li = w.left_idx + row * J, *ri = w.right_idx + row * J;
  const T *lv = pc_ptr<T>(w.left_vals) + row * J, *rv = pc_ptr<T>(w.right_vals) + row * J;
  T l = T(0), r = T(0);
  for (int j = 0; j < J; ++j) {
    const T lt = (li[j] >= 0 && li[j] < M) ? s * lv[j] : T(0);
    const T rt = (ri[j] >= 0 && ri[j] < M) ? s * rv[j] : T(0);
    l = (j == 0) ? lt : l + lt;
    r = (j == 0) ? rt : r + rt;
  }
  return l * r;
}

template <typename T>
__device__ __forceinline__ T src_entry(const PcDevT<T>& d, const lo_op_desc& tm, int64_t b, int pim, int i);

// entry (i, i) of one term, every kind but LO_OP_LOWRANK_DIAG (k_pc_init squares the staged rows)
template <typename T>
__device__ __forceinline__ T src_diag(const PcDevT<T>& d, const lo_op_desc& op, int64_t b, int i) {
  const T* A0 = pc_ptr<T>(op.A0);
  const T* A1 = pc_ptr<T>(op.A1);
  if (op.kind == LO_OP_DENSE_DIAG) {
    return A0[((size_t)b * d.N + i) * d.N + i];
  } else if (op.kind == LO_OP_CALLBACK) {  // generic operator: A1 = matrix._diagonal(), A0 = the fetched pivot rows
    return A1[(size_t)b * d.N + i];
  } else if (op.kind == LO_OP_HADAMARD_DIAG) {
    const T* fi = A0 + ((size_t)b * d.N + i) * op.R;
    const T* gi = A1 + ((size_t)b * d.N + i) * op.n2;
    return seq_dot(fi, fi, (int)op.R) * seq_dot(gi, gi, (int)op.n2);
  } else if (op.kind == LO_OP_TOEPLITZ_DIAG) {
    return A0[(size_t)b * op.R];
  } else if (op.kind == LO_OP_KERNEL_DIAG) {  // os2 g(0) = os2 (an fp32 kind: the operands are read as float)
    return (T)op.A1[(size_t)b * (op.R + 1) + op.R];
  } else if (op.kind == LO_OP_KERNEL_PARAM_DIAG) {  // os2 g(x, x) = os2 for both families
    return (T)op.A1[(size_t)b * (2 * op.R + 2) + op.R];
  } else if (op.kind == LO_OP_KERNEL_SM_DIAG) {  // sum_q w_q, in ascending q (every envelope and cosine is 1 at tau = 0)
    const int W = 2 * (int)op.R + 1, Q = (int)op.n2;
    const float* th = op.A1 + (size_t)b * Q * W;
    float s = th[0];
    for (int q = 1; q < Q; ++q) s = s + th[(size_t)q * W];
    return (T)s;
  } else if (op.kind == LO_OP_KERNEL_SUM_DIAG) {  // sum_t os2_t, in term order
    const float* th = op.A1 + (size_t)b * op.nterms * (op.R + 1);
    float s = th[op.R];
    for (int t = 1; t < op.nterms; ++t) s = s + th[(size_t)t * (op.R + 1) + op.R];
    return (T)s;
  } else if (op.kind == LO_OP_KERNEL_KRON_DIAG || op.kind == LO_OP_KERNEL_TASK_DIAG) {
    // os2 g(0) Bt[t_i, t_i]: KRON: row i = (point, t_i); TASK: t_i the (clamped) id in the points' last column
    const int D = (int)op.R, nt = op.nterms;
    const int ti = op.kind == LO_OP_KERNEL_KRON_DIAG ? i % nt : tk_task_id(op.A0[((size_t)b * d.N + i) * (D + 1) + D], nt);
    return (T)(op.A1[(size_t)b * (D + 1) + D] * op.task[((size_t)b * nt + ti) * nt + ti]);
  } else if (op.kind == LO_OP_KERNEL_LMC_DIAG) {  // sum_q os2_q B_q[t_i, t_i], in term order (row i = (point, t_i))
    const int D = (int)op.R, nt = op.nterms, Q = (int)((op.n2 >> 16) & 15), ti = i % nt;
    const float* th = op.A1 + (size_t)b * Q * (D + 1);
    const float* bt = op.task + ((size_t)b * Q * nt + ti) * nt + ti;
    float s = th[D] * bt[0];
    for (int q = 1; q < Q; ++q) s = s + th[(size_t)q * (D + 1) + D] * bt[(size_t)q * nt * nt];
    return (T)s;
  } else if (op.kind == LO_OP_KERNEL_GRAD_DIAG) {  // row i = (p, a): os2 for the value, os2 t_a^2 for a derivative
    const int D = (int)op.R, a = i % (D + 1);
    const float* th = op.A1 + (size_t)b * (D + 1);
    return (T)(a == 0 ? th[D] : th[D] * (th[a - 1] * th[a - 1]));
  } else if (op.kind == LO_OP_TOEPLITZ_KRON_DIAG) {
    return grid_t0(grid_cols(d, op.A0, b));
  } else if (op.kind == LO_OP_SKI_DIAG || op.kind == LO_OP_SKI_GRID_DIAG) {
    // the approximate diagonal over the base's constant diagonal t0: t[0], on a grid prod_k t_k[0]
    const T t0 = op.kind == LO_OP_SKI_DIAG ? A0[(size_t)b * op.R] : grid_t0(grid_cols(d, op.A0, b));
    return ski_approx_diag<T>(d.ski, op.R, (int)op.n2, (size_t)b * d.N + i, pc_sqrt<T>(t0));
  } else if (op.kind == LO_OP_SKI_SUM_DIAG) {  // the exact diagonal: entry (i, i) of the row, terms ascending
    return src_entry(d, op, b, i, i);
  } else {
    const int n1 = (int)op.R, n2 = (int)op.n2;
    const int i1 = i / n2, i2 = i % n2;
    return A0[((size_t)b * n1 + i1) * n1 + i1] * A1[((size_t)b * n2 + i2) * n2 + i2];
  }
}

// entry (pim, i) of one term, every kind but LO_OP_LOWRANK_DIAG (whose rows k_pc_update stages in LDS).  The kernel
// kinds are fp32 kinds: their operands are read as float
template <typename T>
__device__ __forceinline__ T src_entry(const PcDevT<T>& d, const lo_op_desc& tm, int64_t b, int pim, int i) {
  const T* A0 = pc_ptr<T>(tm.A0);
  const int N = (int)d.N;
  if (tm.kind == LO_OP_DENSE_DIAG) {
    return A0[((size_t)b * N + pim) * N + i];
  } else if (tm.kind == LO_OP_CALLBACK) {
    return A0[(size_t)b * N + i];  // row pi_m of this member, fetched by the host callback for this pivot
  } else if (tm.kind == LO_OP_HADAMARD_DIAG) {
    const int p = (int)tm.R, q = (int)tm.n2;
    const T* F = A0 + (size_t)b * N * p;
    const T* G = pc_ptr<T>(tm.A1) + (size_t)b * N * q;
    return seq_dot(F + (size_t)pim * p, F + (size_t)i * p, p) * seq_dot(G + (size_t)pim * q, G + (size_t)i * q, q);
  } else if (tm.kind == LO_OP_TOEPLITZ_DIAG) {
    return A0[(size_t)b * tm.R + (pim > i ? pim - i : i - pim)];
  } else if (tm.kind == LO_OP_KERNEL_DIAG) {
    const int D = (int)tm.R;
    const float* th = tm.A1 + (size_t)b * (D + 1);
    const float r2 = kern_r2(tm.A0 + ((size_t)b * N + pim) * D, tm.A0 + ((size_t)b * N + i) * D, th, D);
    return (T)(th[D] * kf_g_rt((int)tm.n2, r2));
  } else if (tm.kind == LO_OP_KERNEL_PARAM_DIAG) {
    const int D = (int)tm.R;
    const float* th = tm.A1 + (size_t)b * (2 * D + 2);
    return (T)(th[D] * kp_g_rt((int)tm.n2, tm.A0 + ((size_t)b * N + pim) * D, tm.A0 + ((size_t)b * N + i) * D, th, D));
  } else if (tm.kind == LO_OP_KERNEL_SM_DIAG) {
    const int D = (int)tm.R, Q = (int)tm.n2;
    const float* th = tm.A1 + (size_t)b * Q * (2 * D + 1);
    return (T)ksm_g_rt(tm.A0 + ((size_t)b * N + pim) * D, tm.A0 + ((size_t)b * N + i) * D, th, D, Q);
  } else if (tm.kind == LO_OP_KERNEL_SUM_DIAG) {  // the same per term over the same points, summed in term order
    const int D = (int)tm.R;
    const float* xp = tm.A0 + ((size_t)b * N + pim) * D;
    const float* xi = tm.A0 + ((size_t)b * N + i) * D;
    float s = 0.0f;
    for (int t = 0; t < tm.nterms; ++t) {
      const float* th = tm.A1 + ((size_t)b * tm.nterms + t) * (D + 1);
      const float kt = th[D] * kf_g_rt((int)((tm.n2 >> (4 * t)) & 15), kern_r2(xp, xi, th, D));
      s = t == 0 ? kt : s + kt;
    }
    return (T)s;
  } else if (tm.kind == LO_OP_KERNEL_KRON_DIAG) {  // pivot (p, tau), entry (j, s): (os2 g(r_pj)) Bt[tau, s]
    const int D = (int)tm.R, nt = tm.nterms;
    const int n = N / nt, pp = pim / nt, tau = pim - pp * nt, jj = i / nt, ss = i - jj * nt;
    const float* th = tm.A1 + (size_t)b * (D + 1);
    const float r2 = kern_r2(tm.A0 + ((size_t)b * n + pp) * D, tm.A0 + ((size_t)b * n + jj) * D, th, D);
    return (T)((th[D] * kf_g_rt((int)tm.n2, r2)) * tm.task[((size_t)b * nt + tau) * nt + ss]);
  } else if (tm.kind == LO_OP_KERNEL_LMC_DIAG) {  // the KERNEL_KRON entry per term over the same points, in term order
    const int D = (int)tm.R, nt = tm.nterms, Q = (int)((tm.n2 >> 16) & 15);
    const int n = N / nt, pp = pim / nt, tau = pim - pp * nt, jj = i / nt, ss = i - jj * nt;
    const float* xp = tm.A0 + ((size_t)b * n + pp) * D;
    const float* xi = tm.A0 + ((size_t)b * n + jj) * D;
    float s = 0.0f;
    for (int q = 0; q < Q; ++q) {
      const float* th = tm.A1 + ((size_t)b * Q + q) * (D + 1);
      const float kq = (th[D] * kf_g_rt((int)((tm.n2 >> (4 * q)) & 15), kern_r2(xp, xi, th, D)))
                       * tm.task[(((size_t)b * Q + q) * nt + tau) * nt + ss];
      s = q == 0 ? kq : s + kq;
    }
    return (T)s;
  } else if (tm.kind == LO_OP_KERNEL_TASK_DIAG) {  // pivot p, entry j: (os2 g(r_pj)) Bt[t_p, t_j], ids in column D
    const int D = (int)tm.R, nt = tm.nterms;
    const float* th = tm.A1 + (size_t)b * (D + 1);
    const float* xp = tm.A0 + ((size_t)b * N + pim) * (D + 1);
    const float* xi = tm.A0 + ((size_t)b * N + i) * (D + 1);
    const int tp = tk_task_id(xp[D], nt), tj = tk_task_id(xi[D], nt);
    return (T)((th[D] * kf_g_rt((int)tm.n2, kern_r2(xp, xi, th, D))) * tm.task[((size_t)b * nt + tp) * nt + tj]);
  } else if (tm.kind == LO_OP_KERNEL_GRAD_DIAG) {  // pivot (p, al), entry (j, be): the block formula of lo_amd.h
    const int D = (int)tm.R, nt = D + 1;
    const int n = N / nt, pp = pim / nt, al = pim - pp * nt, jj = i / nt, be = i - jj * nt;
    const float* th = tm.A1 + (size_t)b * nt;
    const float* xp = tm.A0 + ((size_t)b * n + pp) * D;
    const float* xi = tm.A0 + ((size_t)b * n + jj) * D;
    float r2 = 0.0f, ua = 0.0f, ub = 0.0f;  // the loop of kern_r2, keeping the differences u of the coordinates al, be
    for (int k = 0; k < D; ++k) {
      const float df = xp[k] * th[k] - xi[k] * th[k];
      r2 = r2 + df * df;
      if (k + 1 == al) ua = df;
      if (k + 1 == be) ub = df;
    }
    const float e = th[D] * kf_g_rt(LO_KERNEL_RBF, r2);
    float f;
    if (al == 0) f = be == 0 ? 1.0f : th[be - 1] * ub;
    else if (be == 0) f = -(th[al - 1] * ua);
    else f = (th[al - 1] * th[be - 1]) * ((al == be ? 1.0f : 0.0f) - ua * ub);
    return (T)(e * f);
  } else if (tm.kind == LO_OP_TOEPLITZ_KRON_DIAG) {
    const GridCols<T> g = grid_cols(d, tm.A0, b);
    return grid_base(g, grid_pt(g, pim), grid_pt(g, i));
  } else if (tm.kind == LO_OP_SKI_DIAG) {
    return ski_entry<T, false>(d, tm, (size_t)b, pim, i);
  } else if (tm.kind == LO_OP_SKI_SUM_DIAG) {  // the same row per term, summed in term order
    T tv = T(0);
    for (int p = 0; p < tm.nterms; ++p) {
      const T pv = ski_entry<T, false>(d, tm, (size_t)b * tm.nterms + p, pim, i);
      tv = p == 0 ? pv : tv + pv;
    }
    return tv;
  } else if (tm.kind == LO_OP_SKI_GRID_DIAG) {
    return ski_entry<T, true>(d, tm, (size_t)b, pim, i);
  } else {  // LO_OP_KRON_DIAG: K1[p1, i1] K2[p2, i2]
    const int n1 = (int)tm.R, n2 = (int)tm.n2;
    const int p1 = pim / n2, p2 = pim % n2, i1 = i / n2, i2 = i % n2;
    return A0[((size_t)b * n1 + p1) * n1 + i1] * pc_ptr<T>(tm.A1)[((size_t)b * n2 + p2) * n2 + i2];
  }
}

// Stage the C rows of `np` positions (rows i = perm[j0 + t], or i = j0 + t when perm == nullptr) into LDS with row
// stride R + 1 (conflict-free when every thread then walks its own row), coalesced: consecutive lanes read
// consecutive floats (float4 when R % 4 == 0) of consecutive rows.
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ Cb, int R, const long long* __restrict__ perm,
                                           int j0, int np, T* __restrict__ tile) {
  const int ld = R + 1;
  if (sizeof(T) == 4 && (R & 3) == 0) {
    const int RQ = R >> 2;
    for (int e = threadIdx.x; e < np * RQ; e += kThreads) {
      const int pos = e / RQ, q = e % RQ;
      const int i = perm ? (int)perm[j0 + pos] : j0 + pos;
      const float4 v = *reinterpret_cast<const float4*>(Cb + (size_t)i * R + 4 * q);
      T* t = tile + pos * ld + 4 * q;
      t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    }
  } else {
    for (int e = threadIdx.x; e < np * R; e += kThreads) {
      const int pos = e / R, r = e % R;
      const int i = perm ? (int)perm[j0 + pos] : j0 + pos;
      tile[pos * ld + r] = Cb[(size_t)i * R + r];
    }
  }
}

template <typename T>
__host__ __device__ __forceinline__ int tile_positions(int R) {
  // LDS budget ~48 KiB for the tile: 256 positions for R <= 47 (float), fewer for fat roots
  const int tp = (int)(49152 / sizeof(T)) / (R + 1);
  return tp >= kThreads ? kThreads : (tp < 1 ? 1 : tp);
}

// The walk over the low-rank terms that the kernels and the host's LDS sizing share: positions are walked `tp` at a time,
// few enough for the fattest term's tile (one tile, reused by the terms); Rtot: the pivot rows C[pi_m, :] of all terms
// side by side; Rmax + 1: the widest tile row (-1: no low-rank term, no tile)
struct PcTiles {
  int tp;
  int64_t Rtot, Rmax;
};
template <typename T>
__host__ __device__ __forceinline__ PcTiles pc_tiles(const PcDevT<T>& d) {
  PcTiles w{kThreads, 0, -1};
  for (int it = 0; it < d.nterms; ++it)
    if (d.terms[it].kind == LO_OP_LOWRANK_DIAG) {
      const int64_t R = d.terms[it].R;
      const int tp = tile_positions<T>((int)R);
      w.tp = tp < w.tp ? tp : w.tp;
      w.Rtot += R;
      w.Rmax = R > w.Rmax ? R : w.Rmax;
    }
  return w;
}

// per-slice argmax partial: best (value, position) with the FIRST maximal position winning
template <typename T>
__device__ __forceinline__ void slice_argmax(T bv, int bj, T* vbest, int* jbest, T* out_v, int* out_j) {
  vbest[threadIdx.x] = bv;
  jbest[threadIdx.x] = bj;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (threadIdx.x < h) {
      const T ov = vbest[threadIdx.x + h];
      const int oj = jbest[threadIdx.x + h];
      const T mv = vbest[threadIdx.x];
      const int mj = jbest[threadIdx.x];
      if (oj != 0x7fffffff && (mj == 0x7fffffff || ov > mv || (ov == mv && oj < mj))) {
        vbest[threadIdx.x] = ov;
        jbest[threadIdx.x] = oj;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *out_v = vbest[0];
    *out_j = jbest[0];
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_pc_init(PcDevT<T> d) {
  extern __shared__ unsigned char pc_dyn_smem[];
  T* sh = reinterpret_cast<T*>(pc_dyn_smem);
  __shared__ T red[kThreads];
  __shared__ T vbest[kThreads];
  __shared__ int jbest[kThreads];
  const int s = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int N = (int)d.N;
  const int j0 = s * d.rows, j1 = min(N, j0 + d.rows);
  const int tp = pc_tiles(d).tp;
  T lmax = pc_ninf<T>(), lsum = T(0);
  T bv = pc_ninf<T>();
  int bj = 0x7fffffff;
  for (int t0 = j0; t0 < j1; t0 += tp) {
    const int np = min(tp, j1 - t0);
    const int i = t0 + threadIdx.x;
    T v = T(0);
    for (int it = 0; it < d.nterms; ++it) {
      const lo_op_desc& op = d.terms[it];
      T tv = T(0);
      if (op.kind == LO_OP_LOWRANK_DIAG) {
        const int R = (int)op.R;
        __syncthreads();
        stage_rows(pc_ptr<T>(op.A0) + (size_t)b * N * R, R, nullptr, t0, np, sh);
        __syncthreads();
        if ((int)threadIdx.x < np) {
          const T* row = sh + threadIdx.x * (R + 1);
          tv = seq_dot(row, row, R);                   // (root ** 2).sum(-1), root_linear_operator.py:22-28
        }
      } else if ((int)threadIdx.x < np) {
        tv = src_diag(d, op, b, i);
      }
      v = (it == 0) ? tv : v + tv;                     // sum(op._diagonal() for op in linear_ops), left to right
    }
    if ((int)threadIdx.x < np) {
      d.diag[(size_t)b * N + i] = v;
      d.perm[(size_t)b * N + i] = i;
      lmax = pc_max(lmax, v);
      lsum += pc_abs(v);
      if (v > bv || bj == 0x7fffffff) {  // positions increase with the loop: ties keep the earlier one
        bv = v;
        bj = i;
      }
    }
  }
  const T m = pc_block_max(lmax, red);
  const T t = pc_block_sum(lsum, red);
  if (threadIdx.x == 0) {
    d.part_a[b * d.S + s] = m;
    d.part_b[b * d.S + s] = t;
  }
  slice_argmax(bv, bj, vbest, jbest, &d.arg_v[b * d.S + s], &d.arg_j[b * d.S + s]);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_pc_ctrl0(PcDevT<T> d) {
  for (int64_t b = threadIdx.x; b < d.B; b += kThreads) {
    T m = pc_ninf<T>(), t = T(0);
    for (int s = 0; s < d.S; ++s) {
      m = pc_max(m, d.part_a[b * d.S + s]);
      t += d.part_b[b * d.S + s];
    }
    d.orig[b] = m;           // orig_error = max(diag)                    :43
    d.errors[b] = t / m;     // ||diag||_1 / orig_error                    :44
  }
}

// Decides whether pivot m is taken (loop condition :57) from the errors of pivot m-1, then finishes the argmax over
// the not-yet-pivoted positions from the per-slice partials (FIRST maximal position wins: torch.max on CPU, :61-63),
// swaps the permutation entries (:67-70) and sets L[m, pi_m] = sqrt(max) (:73-74).
template <typename T>
__global__ __launch_bounds__(kThreads) void k_pc_ctrl(PcDevT<T> d, int m) {
  if (d.ctrl->stop) return;
  __shared__ T red[kThreads];
  const int N = (int)d.N;
  if (m > 0) {
    T lmax = pc_ninf<T>(), lnan = T(0);
    for (int64_t b = threadIdx.x; b < d.B; b += kThreads) {
      T t = T(0);
      for (int s = 0; s < d.S; ++s) t += d.part_b[b * d.S + s];
      const T e = t / d.orig[b];                                    // :99
      d.errors[b] = e;
      if (e != e) lnan = T(1);
      lmax = pc_max(lmax, e);
    }
    const T mx = pc_block_max(lmax, red);
    const T anynan = pc_block_sum(lnan, red);
    // torch.max propagates NaN and (NaN > tol) is False -> the reference stops
    const bool cont = (anynan == T(0)) && (mx > d.tol);
    if (!cont) {
      if (threadIdx.x == 0) d.ctrl->stop = 1;
      return;
    }
  }
  if (threadIdx.x == 0) d.ctrl->m = m + 1;
  for (int64_t b = threadIdx.x; b < d.B; b += kThreads) {
    T bv = pc_ninf<T>();
    int bj = 0x7fffffff;
    for (int s = 0; s < d.S; ++s) {
      const T v = d.arg_v[b * d.S + s];
      const int j = d.arg_j[b * d.S + s];
      if (j != 0x7fffffff && (bj == 0x7fffffff || v > bv || (v == bv && j < bj))) {
        bv = v;
        bj = j;
      }
    }
    long long* perm = d.perm + (size_t)b * N;
    const long long old = perm[m];
    const long long piv = perm[bj];
    perm[m] = piv;
    perm[bj] = old;
    d.pim[b] = piv;
    d.maxval[b] = bv;
    d.L[((size_t)b * d.max_rank + m) * N + piv] = pc_sqrt(bv);
  }
}

// Schur update of row m (:77-99) over the positions j > m of this workgroup's slice, plus the slice's argmax
// partial for pivot m + 1.
template <typename T>
__global__ __launch_bounds__(kThreads) void k_pc_update(PcDevT<T> d, int m) {
  if (d.ctrl->stop) return;
  extern __shared__ unsigned char pc_dyn_smem[];  // [max_rank] L[j][pi_m] | [R] C[pi_m,:] | row tile
  T* sh = reinterpret_cast<T*>(pc_dyn_smem);
  __shared__ T red[kThreads];
  __shared__ T vbest[kThreads];
  __shared__ int jbest[kThreads];
  const int s = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int N = (int)d.N;
  const long long* perm = d.perm + (size_t)b * N;
  T* diag = d.diag + (size_t)b * N;
  T* Lb = d.L + (size_t)b * d.max_rank * N;
  const int pim = (int)d.pim[b];
  const T piv = pc_sqrt(d.maxval[b]);
  // shared memory: [max_rank] L[j][pi_m] | per low-rank term its row C[pi_m,:] | one row tile (reused by the terms)
  T* upd = sh;
  T* crow = sh + d.max_rank;
  const PcTiles walk = pc_tiles(d);
  const int tp = walk.tp;
  T* tile = crow + (int)walk.Rtot;
  for (int j = threadIdx.x; j < m; j += kThreads) upd[j] = Lb[(size_t)j * N + pim];
  {
    int off = 0;
    for (int it = 0; it < d.nterms; ++it) {
      const lo_op_desc& tm = d.terms[it];
      if (tm.kind != LO_OP_LOWRANK_DIAG) continue;
      const int R = (int)tm.R;
      for (int r = threadIdx.x; r < R; r += kThreads) crow[off + r] = pc_ptr<T>(tm.A0)[((size_t)b * N + pim) * R + r];
      off += R;
    }
  }
  __syncthreads();
  const int j0 = max(s * d.rows, m + 1), j1 = min(N, (s + 1) * d.rows);
  T lerr = T(0);
  T bv = pc_ninf<T>();
  int bj = 0x7fffffff;
  for (int t0 = j0; t0 < j1; t0 += tp) {
    const int np = min(tp, j1 - t0);
    const bool live = (int)threadIdx.x < np;
    const int j = t0 + threadIdx.x;
    const int i = live ? (int)perm[j] : 0;
    T rowv = T(0);
    int off = 0;
    for (int it = 0; it < d.nterms; ++it) {   // row pi_m of the sum = sum of the terms' rows, left to right
      const lo_op_desc& tm = d.terms[it];
      T tv = T(0);
      if (tm.kind == LO_OP_LOWRANK_DIAG) {
        const int R = (int)tm.R;
        __syncthreads();
        stage_rows(pc_ptr<T>(tm.A0) + (size_t)b * N * R, R, perm, t0, np, tile);
        __syncthreads();
        if (live) tv = seq_dot(crow + off, tile + threadIdx.x * (R + 1), R);
        off += R;
      } else if (live) {
        tv = src_entry(d, tm, b, pim, i);
      }
      rowv = (it == 0) ? tv : rowv + tv;
    }
    if (live) {
      T v = rowv;
      if (m > 0) {
        // :83-89, products and sums in the reference's order; the loads of up to sixteen earlier columns are issued
        // together (a load per trip, each waited for before the next, made the update a chain of HBM latencies)
        T acc = T(0);
        for (int j8 = 0; j8 < m; j8 += 16) {
          T lv[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) lv[u] = (j8 + u < m) ? Lb[(size_t)(j8 + u) * N + i] : T(0);
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (j8 + u < m) acc = (j8 + u == 0) ? upd[0] * lv[0] : acc + upd[j8 + u] * lv[u];
        }
        v = rowv - acc;
      }
      v = v / piv;                                   // :91
      Lb[(size_t)m * N + i] = v;                     // :92
      const T dn = diag[i] - v * v;              // :94-95
      diag[i] = dn;
      lerr += pc_abs(dn);
      if (dn > bv || bj == 0x7fffffff) {
        bv = dn;
        bj = j;
      }
    }
  }
  const T t = pc_block_sum(lerr, red);
  if (threadIdx.x == 0) d.part_b[b * d.S + s] = t;
  slice_argmax(bv, bj, vbest, jbest, &d.arg_v[b * d.S + s], &d.arg_j[b * d.S + s]);
}

template <typename T>
static void pc_layout(const lo_op_desc* op, int max_rank, Arena& ar, PcDevT<T>* d) {
  const int64_t B = op->B, N = op->N;
  Split sp = choose_split(B, N, 1024);
  d->op = *op;
  if (op->kind == LO_OP_SUM) {
    d->nterms = op->terms ? std::min<int>(std::max<int>(op->nterms, 0), LO_MAX_TERMS) : 0;
    for (int i = 0; i < d->nterms; ++i) d->terms[i] = op->terms[i];
  } else {
    d->nterms = 1;
    d->terms[0] = *op;
  }
  const bool ski = op->kind == LO_OP_SKI_DIAG || op->kind == LO_OP_SKI_GRID_DIAG || op->kind == LO_OP_SKI_SUM_DIAG;
  d->ski = (ski && op->interp) ? *op->interp : lo_interp_desc{};
  if (op->kind == LO_OP_TOEPLITZ_KRON_DIAG && op->grid) {
    d->ski.grid_ndim = op->grid->ndim;
    for (int k = 0; k < 3; ++k) d->ski.grid_m[k] = op->grid->m[k];
  }
  d->B = B; d->N = N; d->S = sp.S; d->rows = sp.rows; d->max_rank = max_rank;
  d->ctrl = ar.take<PcCtrl>(1);
  d->diag = ar.take<T>((size_t)B * N);
  d->pim = ar.take<long long>(B);
  d->maxval = ar.take<T>(B);
  d->part_a = ar.take<T>((size_t)B * sp.S);
  d->part_b = ar.take<T>((size_t)B * sp.S);
  d->orig = ar.take<T>(B);
  d->errors = ar.take<T>(B);
  d->arg_v = ar.take<T>((size_t)B * sp.S);
  d->arg_j = ar.take<int>((size_t)B * sp.S);
}

typedef int (*pc_rowfetch_any)(void* user, const int64_t* piv, void* rows, int64_t B, int64_t N, void* stream);

// streaming engine shared by the descriptor and the callback entry points, float and double
template <typename T>
static int pc_stream_t(const lo_op_desc* op, const T* diag0, pc_rowfetch_any row_cb, void* row_user, int32_t max_rank,
                       T error_tol, T* L_rows, int64_t* perm, int32_t* rank_out, void* ws, size_t ws_bytes,
                       hipStream_t st) {
  const int64_t B = op->B, N = op->N;
  const int rank = (int)std::min<int64_t>(max_rank, N);  // :33
  Arena ar(ws, ws_bytes);
  PcDevT<T> d;
  pc_layout(op, max_rank, ar, &d);
  if (row_cb) {  // generic operator: one "term" whose rows arrive through the callback
    T* rows = ar.take<T>((size_t)B * N);
    d.terms[0].A0 = reinterpret_cast<const float*>(rows);
    d.terms[0].A1 = reinterpret_cast<const float*>(diag0);
  }
  if (!ar.ok) return LO_ERR_WORKSPACE;
  d.tol = error_tol;
  d.L = L_rows;
  d.perm = (long long*)perm;
  LO_HIP_CHECK(hipMemsetAsync(d.ctrl, 0, sizeof(PcCtrl), st));
  LO_HIP_CHECK(hipMemsetAsync(L_rows, 0, sizeof(T) * (size_t)B * max_rank * N, st));  // L = zeros :36-42
  dim3 grid(d.S, (unsigned)B), block(kThreads);
  // shared memory: the pivot rows of all low-rank terms (R elements in total) + one row tile sized for the walk of the
  // fattest low-rank term (pc_tiles: the walk the kernels make)
  const PcTiles walk = pc_tiles(d);
  const size_t R = (size_t)walk.Rtot, tile_elems = (size_t)walk.tp * (size_t)(walk.Rmax + 1);
  if ((tile_elems + R + max_rank) * sizeof(T) > 60000) return LO_ERR_UNSUPPORTED;
  LO_PROF_BEGIN("pc_init", st);
  hipLaunchKernelGGL((k_pc_init<T>), grid, block, tile_elems * sizeof(T), st, d);
  LO_PROF_END(st);
  hipLaunchKernelGGL((k_pc_ctrl0<T>), dim3(1), block, 0, st, d);
  LO_LAUNCH_CHECK();
  for (int m = 0; m < rank; ++m) {
    LO_PROF_BEGIN("pc_ctrl_argmax", st);
    hipLaunchKernelGGL((k_pc_ctrl<T>), dim3(1), block, 0, st, d, m);
    LO_PROF_END(st);
    if (m + 1 < N) {  // :77
      if (row_cb) {  // row = matrix[..., pi_m, :] (:81): the reference's generic __getitem__, as a callback
        if (row_cb(row_user, (const int64_t*)d.pim, const_cast<float*>(d.terms[0].A0), B, N, (void*)st))
          return LO_ERR_LAUNCH;
      }
      LO_PROF_BEGIN("pc_update", st);
      hipLaunchKernelGGL((k_pc_update<T>), grid, block, (max_rank + R + tile_elems) * sizeof(T), st, d, m);
      LO_PROF_END(st);
    }
    LO_LAUNCH_CHECK();
  }
  PcCtrl h;
  LO_HIP_CHECK(hipMemcpyAsync(&h, d.ctrl, sizeof(PcCtrl), hipMemcpyDeviceToHost, st));
  LO_HIP_CHECK(hipStreamSynchronize(st));
  *rank_out = h.m;
  return LO_OK;
}

// the descriptor of a generic operator whose rows and diagonal arrive through callbacks
static lo_op_desc pc_cb_desc(int64_t B, int64_t N) {
  lo_op_desc op;
  memset(&op, 0, sizeof(op));
  op.kind = LO_OP_CALLBACK; op.B = B; op.N = N;
  return op;
}

template <typename T>
static size_t pc_ws_bytes(const lo_op_desc* op, int32_t max_rank, bool cb) {
  PcDevT<T> d;
  return measured(1024, [&](Arena& ar) {
    pc_layout(op, max_rank, ar, &d);
    if (cb) ar.take<T>((size_t)op->B * op->N);  // the fetched rows
  });
}

// One *_desc_check per kind (lo_internal.h), shared with the kind's plan function; the streaming engine reads single
// entries, so it adds none of the products' shape bounds.  fp32_kinds: the caller reads the operands as float (the
// float64 engine takes the plain kinds and sums of them only)
static int pc_check_desc(const lo_op_desc* op, bool fp32_kinds = true) {
  int rc = LO_OK;
  switch (op->kind) {
    case LO_OP_LOWRANK_DIAG: case LO_OP_DENSE_DIAG: case LO_OP_KRON_DIAG: break;
    case LO_OP_SUM:
      if (op->nterms < 2 || op->nterms > LO_MAX_TERMS || !op->terms) return LO_ERR_BADARG;
      for (int i = 0; i < op->nterms; ++i) {
        const lo_op_desc& t = op->terms[i];
        if (!(plain_term_kind(t.kind) || kernel_term_kind(t.kind)) || t.B != op->B || t.N != op->N) return LO_ERR_BADARG;
        if (kernel_term_kind(t.kind)) {  // (a term is validated as the kind on its own is)
          if (!fp32_kinds) return LO_ERR_UNSUPPORTED;
          if (t.kind == LO_OP_KERNEL_DIAG) rc = kernel_desc_check(&t);
          else if (t.kind == LO_OP_KERNEL_SM_DIAG) rc = kernel_sm_desc_check(&t);
          else rc = t.kind == LO_OP_KERNEL_PARAM_DIAG ? kernel_param_desc_check(&t) : kernel_sum_desc_check(&t);
          if (rc) return rc;
        }
      }
      break;
    case LO_OP_HADAMARD_DIAG: rc = hadamard_desc_check(op); break;
    case LO_OP_TOEPLITZ_DIAG: rc = toeplitz_desc_check(op); break;
    case LO_OP_TOEPLITZ_KRON_DIAG: rc = toeplitz_kron_desc_check(op); break;
    case LO_OP_KERNEL_DIAG: rc = kernel_desc_check(op); break;
    case LO_OP_KERNEL_SUM_DIAG: rc = kernel_sum_desc_check(op); break;
    case LO_OP_KERNEL_KRON_DIAG: rc = kernel_kron_desc_check(op); break;
    case LO_OP_KERNEL_LMC_DIAG: rc = kernel_lmc_desc_check(op); break;
    case LO_OP_KERNEL_GRAD_DIAG: rc = kernel_grad_desc_check(op); break;
    case LO_OP_KERNEL_TASK_DIAG: rc = kernel_task_desc_check(op); break;
    case LO_OP_KERNEL_PARAM_DIAG: rc = kernel_param_desc_check(op); break;
    case LO_OP_KERNEL_SM_DIAG: rc = kernel_sm_desc_check(op); break;
    case LO_OP_SKI_DIAG: rc = ski_desc_check(op); break;
    case LO_OP_SKI_SUM_DIAG: rc = ski_sum_desc_check(op); break;
    // (an empty grid or stencil is refused here ahead of the grid shape; the plan refuses it behind, as a shape)
    case LO_OP_SKI_GRID_DIAG: rc = (op->R < 1 || op->n2 < 1) ? LO_ERR_BADARG : ski_grid_desc_check(op); break;
    default: return LO_ERR_UNSUPPORTED;
  }
  if (rc) return rc;
  return op->N > 0x7ffffff0 ? LO_ERR_UNSUPPORTED : LO_OK;
}

}  // namespace lo

using namespace lo;

extern "C" {

size_t lo_pivoted_cholesky_workspace_bytes(const lo_op_desc* op, int32_t max_rank) {
  if (!op) return 0;
  size_t need = std::max(pc_ws_bytes<float>(op, max_rank, false),
                         (pc_onchip_eligible(op, max_rank) ? pc_onchip_workspace_bytes(op, max_rank) : (size_t)0));
  if (pc_onchip_rows_eligible(op, max_rank)) need = std::max(need, pc_onchip_rows_workspace_bytes(op, max_rank));
  return need;
}

int lo_pivoted_cholesky_f32(const lo_op_desc* op, int32_t max_rank, float error_tol, float* L_rows, int64_t* perm,
                            int32_t* rank_out, void* ws, size_t ws_bytes, void* stream) {
  if (!op || !L_rows || !perm || !rank_out || !ws || max_rank < 1) return LO_ERR_BADARG;
  if (const int rc = pc_check_desc(op)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int rank = (int)std::min<int64_t>(max_rank, op->N);  // :33
  resident_tick();
  if (pc_onchip_eligible(op, max_rank)) {  // operator-resident fast path (lo_pivchol_onchip.hip), same results
    const int rc = pc_onchip_run(op, rank, max_rank, error_tol, L_rows, (long long*)perm, rank_out, ws, ws_bytes, st);
    if (rc != LO_ERR_LAUNCH) return rc;
    (void)hipGetLastError();  // exchange timed out (co-residency lost): redo with the streaming engine
  } else if (pc_onchip_rows_eligible(op, max_rank)) {  // dense / Kronecker rows, same results (k_pc_onchip_rows)
    const int rc = pc_onchip_rows_run(op, rank, max_rank, error_tol, L_rows, (long long*)perm, rank_out, ws, ws_bytes, st);
    if (rc != LO_ERR_LAUNCH) return rc;
    (void)hipGetLastError();
  }
  return pc_stream_t<float>(op, nullptr, nullptr, nullptr, max_rank, error_tol, L_rows, perm, rank_out, ws, ws_bytes, st);
}

size_t lo_pivoted_cholesky_cb_workspace_bytes(int64_t B, int64_t N, int32_t max_rank) {
  const lo_op_desc op = pc_cb_desc(B, N);
  return pc_ws_bytes<float>(&op, max_rank, true);
}

int lo_pivoted_cholesky_cb_f32(int64_t B, int64_t N, const float* diag, lo_rowfetch_cb row_cb, void* row_user,
                               int32_t max_rank, float error_tol, float* L_rows, int64_t* perm, int32_t* rank_out,
                               void* ws, size_t ws_bytes, void* stream) {
  if (!diag || !row_cb || !L_rows || !perm || !rank_out || !ws || max_rank < 1 || B < 1 || N < 1) return LO_ERR_BADARG;
  if (N > 0x7ffffff0) return LO_ERR_UNSUPPORTED;
  const lo_op_desc op = pc_cb_desc(B, N);
  return pc_stream_t<float>(&op, diag, reinterpret_cast<pc_rowfetch_any>(row_cb), row_user, max_rank, error_tol, L_rows,
                            perm, rank_out, ws, ws_bytes, (hipStream_t)stream);
}

// ---- float64 (round 4): the reference's PivotedCholesky.forward is dtype-generic.  Same streaming engine, same
// operation order; the descriptor's pointers (A0, A1; d is ignored) are read as `const double*`.
size_t lo_pivoted_cholesky_f64_workspace_bytes(const lo_op_desc* op, int32_t max_rank) {
  return op ? pc_ws_bytes<double>(op, max_rank, false) : 0;
}

int lo_pivoted_cholesky_f64(const lo_op_desc* op, int32_t max_rank, double error_tol, double* L_rows, int64_t* perm,
                            int32_t* rank_out, void* ws, size_t ws_bytes, void* stream) {
  if (!op || !L_rows || !perm || !rank_out || !ws || max_rank < 1) return LO_ERR_BADARG;
  // the kinds whose operands may be doubles; every other kind would have its floats read as doubles
  if (!(plain_term_kind(op->kind) || op->kind == LO_OP_SUM)) return LO_ERR_UNSUPPORTED;
  if (const int rc = pc_check_desc(op, false)) return rc;
  return pc_stream_t<double>(op, nullptr, nullptr, nullptr, max_rank, error_tol, L_rows, perm, rank_out, ws, ws_bytes,
                             (hipStream_t)stream);
}

size_t lo_pivoted_cholesky_cb_f64_workspace_bytes(int64_t B, int64_t N, int32_t max_rank) {
  const lo_op_desc op = pc_cb_desc(B, N);
  return pc_ws_bytes<double>(&op, max_rank, true);
}

int lo_pivoted_cholesky_cb_f64(int64_t B, int64_t N, const double* diag, lo_rowfetch_cb_f64 row_cb, void* row_user,
                               int32_t max_rank, double error_tol, double* L_rows, int64_t* perm, int32_t* rank_out,
                               void* ws, size_t ws_bytes, void* stream) {
  if (!diag || !row_cb || !L_rows || !perm || !rank_out || !ws || max_rank < 1 || B < 1 || N < 1) return LO_ERR_BADARG;
  if (N > 0x7ffffff0) return LO_ERR_UNSUPPORTED;
  const lo_op_desc op = pc_cb_desc(B, N);
  return pc_stream_t<double>(&op, diag, reinterpret_cast<pc_rowfetch_any>(row_cb), row_user, max_rank, error_tol, L_rows,
                             perm, rank_out, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
