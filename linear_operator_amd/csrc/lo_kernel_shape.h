// lo_kernel_shape.h -- the host side that every kind of the matrix-free kernel family shares (lo_kernel_op.hip and its
// float64 twin, lo_kernel_sum.hip, lo_kernel_kron.hip, lo_kernel_lmc.hip, lo_kernel_grad.hip, lo_kernel_task.hip):
// argument checks, the launch shape, the padded sizes, the choice of a kernel instantiation from run-time values
// (ko_pick / ko_dispatch), the layout of a split member's partials and their reduction.  No device code lives here.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "lo_internal.h"

namespace lo {

constexpr int kKoTJ = 128;  // points of x2 per LDS tile
constexpr int kKoTS = 8;    // columns s of U / V per sweep of the derivative
constexpr int kKoMaxSplit = 64;
constexpr size_t kKoTail = 256;  // what the sizers report beyond the layout

struct KoShape {
  int rb;       // row blocks of 256
  int js;       // workgroups a member's columns j are split over
  int jchunk;   // columns per split (a multiple of kKoTJ)
};

inline bool ko_args_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t c) {
  return B >= 1 && M >= 1 && N >= 1 && D >= 1 && c >= 1;
}
inline bool ko_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D) {
  return D <= LO_KERNEL_MAX_DIM && B <= 65535 && M <= 0x7ffffe00 && N <= 0x7ffffe00;
}
inline bool ko_family_ok(int64_t family) { return family >= LO_KERNEL_RBF && family <= LO_KERNEL_MATERN52; }

// the diagonal operand of a product's entry point: a known mode, and d wherever the term is applied (`square`: M == N;
// the kinds that apply it to a rectangular operator drop the mode instead)
inline bool ko_diag_ok(int diag_mode, const void* d, bool square) {
  if (diag_mode != LO_DIAG_NONE && diag_mode != LO_DIAG_FULL && diag_mode != LO_DIAG_CONST) return false;
  return diag_mode == LO_DIAG_NONE || !square || d;
}

inline KoShape ko_shape(int64_t B, int64_t M, int64_t N) {
  KoShape s;
  s.rb = (int)((M + kThreads - 1) / kThreads);
  const int64_t wgs = (int64_t)s.rb * B;
  const int64_t tiles = (N + kKoTJ - 1) / kKoTJ;
  int64_t js = 1;
  if (wgs < 512) js = std::min<int64_t>(std::min<int64_t>(tiles, (512 + wgs - 1) / wgs), kKoMaxSplit);
  const int64_t per = (tiles + js - 1) / js;
  s.jchunk = (int)(per * kKoTJ);
  s.js = (int)((N + s.jchunk - 1) / s.jchunk);
  return s;
}

inline int ko_padded_dim(int64_t D) { return D <= 4 ? 4 : (D <= 8 ? 8 : (D <= 16 ? 16 : 32)); }
inline int ko_col_chunk(int64_t c) { return c == 1 ? 1 : (c <= 4 ? 4 : 16); }
using ko_cols = std::integer_sequence<int, 1, 4, 16>;  // what ko_col_chunk yields

// what a sweep's launch is made of: the shape, the padded dimension and the grid (row blocks, B, js)
struct KoSweep {
  KoShape s;
  int DP;
  dim3 grid;
  KoSweep(int64_t B, int64_t M, int64_t N, int64_t D)
      : s(ko_shape(B, M, N)), DP(ko_padded_dim(D)), grid((unsigned)s.rb, (unsigned)B, (unsigned)s.js) {}
};

// The one layout of a split member's partials, [js, B, rows, cols] of T when ko_shape(B, rows, N).js > 1 (else nothing):
// every sizer, plan and entry point of the family lays them out through this function.
template <class T>
inline T* ko_split_layout(Arena& ar, int64_t B, int64_t rows, int64_t N, int64_t cols) {
  const KoShape s = ko_shape(B, rows, N);
  return s.js > 1 ? ar.take<T>((size_t)s.js * B * rows * cols) : nullptr;
}

// the one layout of a bilinear sweep's workspace: a partial [DP + 1] per workgroup, [B, rb js, DP + 1] (ko_bil_reduce)
template <class T>
inline T* ko_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<T>((size_t)B * s.rb * s.js * (ko_padded_dim(D) + 1));
}

// f(std::integral_constant<int, V>) for the first V of the list that equals v, else for the last one (the `default:` arm)
template <class F, int V0, int... Vs>
inline void ko_pick(std::integer_sequence<int, V0, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) {
    f(std::integral_constant<int, V0>{});
  } else {
    if (v == V0) f(std::integral_constant<int, V0>{});
    else ko_pick(std::integer_sequence<int, Vs...>{}, v, f);
  }
}
using ko_families =
    std::integer_sequence<int, LO_KERNEL_RBF, LO_KERNEL_MATERN12, LO_KERNEL_MATERN32, LO_KERNEL_MATERN52>;
using ko_dims = std::integer_sequence<int, 4, 8, 16, 32>;  // what ko_padded_dim yields

// f(family, padded dimension[, column chunk]) as integral constants: the instantiation of a kernel template <F, DP[, CC]>
template <class F>
inline void ko_dispatch(int family, int DP, F&& f) {
  ko_pick(ko_families{}, family, [&](auto fam) { ko_pick(ko_dims{}, DP, [&](auto dp) { f(fam, dp); }); });
}
template <class Cols, class F>
inline void ko_dispatch(int family, int DP, Cols cols, int CC, F&& f) {
  ko_dispatch(family, DP, [&](auto fam, auto dp) { ko_pick(cols, CC, [&](auto cc) { f(fam, dp, cc); }); });
}

// ---- the column chunks of the other kinds: what a sweep of the product carries, and the list ko_pick chooses from --------
// Kronecker (lo_kernel_kron.hip), by the wide column count W = T c
inline int kk_col_chunk(int64_t W) { return W <= 4 ? 4 : (W <= 16 ? 16 : 32); }
using kk_cols = std::integer_sequence<int, 4, 16, 32>;
// the tasks and the sizes the kinds with a task factor take (lo_kernel_kron.hip, lo_kernel_lmc.hip): what both the entry
// point and the descriptor are held to (B, n, D, T, c already positive)
inline bool kk_tasks_ok(int64_t T) { return T >= 1 && T <= LO_KERNEL_KRON_MAX_TASKS; }
inline bool kk_shape_ok(int64_t B, int64_t n, int64_t D, int64_t T, int64_t c) {
  return ko_shape_ok(B, n, n, D) && n * T <= 0x7ffffe00 && T * c <= 0x7fffffff;
}
// LMC (lo_kernel_lmc.hip), by the terms Q and the wide column count: Q copies of the tile of B_q v sit in LDS next to Q
// copies of the scaled points, so three and four terms carry at most 8 wide columns per sweep (64 KB per workgroup)
inline int kl_col_chunk(int64_t Q, int64_t W) { return W <= 4 ? 4 : ((W <= 8 || Q > 2) ? 8 : 16); }
using kl_cols = std::integer_sequence<int, 4, 8, 16>;

// float64 (lo_kernel_op_f64.hip): 1 / 4 / 8 (DP = 32: 1 / 4 -- the point alone is 64 VGPRs there)
inline int ko64_col_chunk(int64_t c, int DP) { return c == 1 ? 1 : ((c <= 4 || DP == 32) ? 4 : 8); }
template <int DP>
using ko64_cols = std::conditional_t<DP == 32, std::integer_sequence<int, 1, 4>, std::integer_sequence<int, 1, 4, 8>>;
// float64, many columns (lo_kernel_mv_wide_f64.hip): 16-column tiles NT per sweep.  The tile of points (DP KB) and of v
// (16 NT KB) are the workgroup's LDS, 64 KB at most: three tiles, two at DP = 32.  The sweeps are made even: 17 columns
// are one sweep of two tiles, 65 two sweeps of three (three of two at DP = 32).
constexpr int ko64_wide_max_tiles(int DP) { return DP == 32 ? 2 : 3; }
inline int ko64_wide_tiles(int64_t c, int DP) {
  const int64_t tiles = (c + 15) / 16, most = ko64_wide_max_tiles(DP);
  const int64_t sweeps = (tiles + most - 1) / most;
  return (int)((tiles + sweeps - 1) / sweeps);
}
template <int DP>
using ko64_wide_nts = std::conditional_t<DP == 32, std::integer_sequence<int, 1, 2>, std::integer_sequence<int, 1, 2, 3>>;
// Which of the two kernel_mv_run_f64 launches (lo_kernel_op_f64.hip): a function of the column count and the padded
// dimension alone, read by kernel_mv_run_f64 and nothing else.  The cells come from the column sweep of
// tools/mb_kernel_f64.py --what wide: a cell is routed to k64_kernel_mv_wide only where its slowest
// round beat k64_kernel_mv's fastest.  From 9 columns on (a second sweep of k64_kernel_mv) it won in every cell, 0.48 - 0.66
// of the time at 9 .. 16 columns, 0.14 - 0.56 from 17 on; at 5 .. 8 columns (two sweeps of four at DP 32) it won at DP 32
// (0.59 - 0.60), lost at DP 4 and 8 (1.12 - 1.31) and split at DP 16 (0.94 - 1.20: not routed); up to 4 columns
// k64_kernel_mv is kept everywhere (1.16 - 1.56), c = 1 included, which tests/test_gpu_kernel_variants.py pins by name.
inline bool ko64_wide(int64_t c, int DP) { return c >= 9 || (c >= 5 && DP == 32); }
// y[b, i, col] = [y +] sum_z part[z, b, i, col] (ascending z) + d o v over `total` = B rows c doubles (lo_kernel_op_f64.hip)
int ko64_reduce_splits(const char* prof_name, const double* part, int js, size_t per_member, size_t total, int c,
                       const double* d, int dmode, int accumulate, const double* v, double* y, hipStream_t st);
// g_theta [B, D + 1] from the per-workgroup partials [B, nblk, DP + 1] of a float64 bilinear sweep, in ascending order
// (lo_kernel_op_f64.hip, k64_kernel_bil_reduce): slot q < D times os2 / theta[q], slot DP as it is
int ko64_bil_reduce(const double* part, int nblk, int DP, int64_t B, int64_t D, const double* theta, double* g_theta,
                    hipStream_t st);
// waves per SIMD the float64 derivative kernels are held to (the second argument of __launch_bounds__, i.e.
// amdgpu_waves_per_eu): two (<= 256 VGPRs) up to DP = 16; at DP = 32 the point, the running and the tile sums are 192 VGPRs
// before anything else, so one wave per SIMD, whose budget of 512 lets the accumulation registers hold what does not fit
template <int DP>
constexpr int ko64_waves() {
  return DP == 32 ? 1 : 2;
}
// columns of U / V one sweep of the float64 wide derivatives carries (lo_kernel_bil_wide_f64.hip): the contraction length
// of W = U V^T on v_mfma_f64_16x16x4_f64.  A lane keeps 2 cols VGPRs of B operands beside the 32 of the accumulators and
// the 6 DP of its point, running and tile sums; the V tile is 1.125 cols KB of LDS beside DP KB of points.  The largest
// multiple of 4 at which none of the 8 instantiations of a DP uses scratch under ko64_waves: 64 KB
// of static LDS end DP 4, 8 and 32 (64064 / 63584 / 65312 bytes); registers end DP 16, where Matern-1/2's hyperparameter
// kernel spills 20 bytes per lane at 20 columns (the other seven take 20, and 24 with 12 - 20 bytes in three of them)
constexpr int ko64_bil_wide_cols(int DP) { return DP <= 4 ? 52 : (DP <= 8 ? 48 : (DP <= 16 ? 16 : 28)); }
// Which of the two kernel_bil_run_f64 and kernel_pgrad_run_f64 launch: a function of the column count and the padded
// dimension alone, read by those two and nothing else.  The cells come from the derivative sweep of tools/mb_kernel_f64.py
// --what wide_derivs: a cell is routed to k64_kernel_bil_wide only where its slowest round beat the
// plain kernel's fastest.  From 9 columns on (a second sweep of the plain kernels at DP <= 8) it won in every cell of both
// kernels: 0.56 - 0.65 of the time at 9 .. 16 columns and 0.27 - 0.46 from 17 on at DP 4 and 8, 0.30 - 0.47 at DP 16,
// 0.11 - 0.33 at DP 32.  At 5 .. 8 columns it won at DP 16 (0.56 - 0.60: two sweeps of four) and DP 32 (0.27 - 0.53: three
// or four sweeps of two) and lost at DP 4 and 8 (1.05 - 1.12: one sweep either way).  t <= 4 always stays on k64_kernel_bil
// / k64_kernel_pgrad, which tests/test_gpu_kernel_variants.py pins by name.
inline bool ko64_bil_wide(int64_t t, int DP) { return t >= 9 || (t >= 5 && DP >= 16); }

// gradient kernel (lo_kernel_grad.hip), by the padded dimension: a thread holds (DP + 1) CC running sums and as many tile
// sums, and every instantiation stays at 3 waves per SIMD (<= 168 VGPRs) without scratch -- 4 columns at DP 4, 2 at DP 8, 1
// at DP 16 (one more column at DP 8 / 16 spills: 200 / 249 VGPRs unconstrained)
inline int kg_col_chunk(int DP, int64_t c) {
  const int most = DP <= 4 ? 4 : (DP <= 8 ? 2 : 1);
  return c == 1 ? 1 : (c == 2 ? std::min(most, 2) : most);
}
using kg_dims = std::integer_sequence<int, 4, 8, 16>;  // ko_padded_dim up to LO_KERNEL_GRAD_MAX_DIM
template <int DP>
using kg_cols = std::conditional_t<DP <= 4, std::integer_sequence<int, 4, 2, 1>,
                                   std::conditional_t<DP <= 8, std::integer_sequence<int, 2, 1>, std::integer_sequence<int, 1>>>;
// columns of U / V one sweep of its derivative carries: the thread keeps DP + 1 scaled entries of U per column in registers
constexpr int kg_bil_cols(int DP) { return DP <= 4 ? kKoTS : (DP <= 8 ? 4 : 2); }
// columns of U / V one sweep of the plain kind's wide derivatives carries (lo_kernel_bil_wide.hip): the contraction length
// of W = U V^T on the matrix cores, half of them per lane in registers for each of two rows, beside the lane's point, its
// DP running and DP tile sums and the 32 accumulators of W
constexpr int ko_bil_wide_cols(int DP) { return 32; }

// Matern-5/2 gradient kernel (lo_kernel_mgrad.hip), by the padded dimension (kg_dims): the sums of the RBF gradient kernel
// plus three radial factors instead of one, and every instantiation still stays at 3 waves per SIMD without scratch
// (product: 61 / 76 / 110 VGPRs at DP 4, 95 / 124 at DP 8, 167 at DP 16; derivative: 162 / 161 / 164)
inline int km_col_chunk(int DP, int64_t c) { return kg_col_chunk(DP, c); }
template <int DP>
using km_cols = kg_cols<DP>;
constexpr int km_bil_cols(int DP) { return DP <= 4 ? kKoTS : (DP <= 8 ? 4 : 2); }

// the single-term product on validated arguments (lo_kernel_op.hip); tstride: floats between two members' thetas;
// part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
int kernel_mv_run(const float* x1, const float* x2, const float* theta, int64_t tstride, int family, int64_t B, int64_t M,
                  int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                  const int* stop, hipStream_t st);

// The many-column product on the matrix cores (lo_kernel_mv_wide.hip, k_kernel_mv_wide): same arguments, same partials.
int kernel_mv_wide_run(const float* x1, const float* x2, const float* theta, int64_t tstride, int family, int64_t B,
                       int64_t M, int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y,
                       float* part, const int* stop, hipStream_t st);
// Which of the two kernel_mv_run launches: a function of the column count and the padded dimension alone, read by
// kernel_mv_run and nothing else.  The cells come from the column sweep of tools/mb_kernel_op.py:
// a cell is routed to k_kernel_mv_wide only where its median beat k_kernel_mv's by more than the measured spread.  From 17
// columns on (a second sweep of k_kernel_mv) it won at every DP, 0.34 - 0.77 of the time; at 5 .. 16 columns it won at
// DP 16 and 32 (0.66 - 0.83) and lost at DP 4 and 8 (1.02 - 1.14); up to 4 columns k_kernel_mv is kept everywhere.
inline bool ko_wide(int64_t c, int DP) { return c >= 17 || (c >= 5 && DP >= 16); }

// The derivatives of sum_s u_s^T K(x1, x2) v_s on validated arguments (lo_kernel_op.hip): the hyperparameters, part the
// partials of ko_bil_layout, and the points x1, part the partials of ko_split_layout with D columns
int kernel_bil_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M, int64_t N,
                   int64_t D, const float* U, const float* V, int64_t t, float* g_theta, float* part, hipStream_t st);
int kernel_pgrad_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M, int64_t N,
                     int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part, hipStream_t st);
// The same with W = U V^T on the matrix cores (lo_kernel_bil_wide.hip, k_kernel_bil_wide): same arguments, same partials.
int kernel_bil_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M, int64_t N,
                        int64_t D, const float* U, const float* V, int64_t t, float* g_theta, float* part, hipStream_t st);
int kernel_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                          int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                          hipStream_t st);
// Which of the two kernel_bil_run and kernel_pgrad_run launch: a function of the column count and the padded dimension
// alone, read by those two and nothing else.  The cells come from the derivative sweep of tools/mb_kernel_op.py (--what
// bilwide): from 9 columns on (a second sweep of the old kernels) k_kernel_bil_wide's slowest round
// beat the old kernel's fastest in every cell of both kernels, 0.43 - 0.57 of the time at 9 .. 16 columns and 0.28 - 0.45
// from 17 on.  Up to 8 columns it also won in all cells but one (0.76 - 0.94 at DP <= 16, 0.95 - 1.01 at DP 32; the points'
// kernel at DP 32, t = 8 lost); those cells keep the old kernels, as ko_wide keeps c <= 4: the few-column derivatives of
// every caller stay the kernels they were, which tests/test_gpu_kernel_variants.py pins by name.
inline bool ko_bil_wide(int64_t t, int DP) { return t >= 9; }

// ---- the kinds with a pair value of their own: rational quadratic / periodic (lo_kernel_param.hip) and spectral mixture
// (lo_kernel_sm.hip); what their entry points and those of lo_kernel_kinds_wide.hip are held to ---------------------------
inline bool kp_family_ok(int64_t family) { return family == LO_KERNEL_RQ || family == LO_KERNEL_PERIODIC; }
inline bool kp_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D) {
  return D <= LO_KERNEL_PARAM_MAX_DIM && ko_shape_ok(B, M, N, D);
}
using kp_families = std::integer_sequence<int, LO_KERNEL_RQ, LO_KERNEL_PERIODIC>;
template <class F>
inline void kp_dispatch(int family, int DP, F&& f) {
  ko_pick(kp_families{}, family, [&](auto fam) { ko_pick(ko_dims{}, DP, [&](auto dp) { f(fam, dp); }); });
}
inline bool ksm_args_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  return ko_args_ok(B, M, N, D, c) && Q >= 1;
}
inline bool ksm_shape_ok(int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q, int64_t c) {
  return D <= LO_KERNEL_SM_MAX_DIM && Q <= LO_KERNEL_SM_MAX_MIX && ko_shape_ok(B, M, N, D) && c <= 0x7fffffff;
}
using ksm_dims = std::integer_sequence<int, 4, 8, 16>;  // ko_padded_dim up to LO_KERNEL_SM_MAX_DIM
// the diagonal operand of both kinds' products: ko_diag_ok, and no mode at all on a rectangular product
inline bool kp_diag_ok(int diag_mode, const void* d, bool square) {
  return ko_diag_ok(diag_mode, d, square) && (square || diag_mode == LO_DIAG_NONE);
}
inline bool ksm_diag_ok(int diag_mode, const void* d, bool square) { return kp_diag_ok(diag_mode, d, square); }

// Their many-column products on the matrix cores (lo_kernel_kinds_wide.hip, k_kinds_mv_wide): the arguments and the
// partials of kernel_param_mv_run / kernel_sm_mv_run.
int kernel_param_mv_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                             int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y,
                             float* part, const int* stop, hipStream_t st);
int kernel_sm_mv_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                          int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                          const int* stop, hipStream_t st);
// Which of the two kernel_param_mv_run and kernel_sm_mv_run launch: functions of the family, the column count and the
// padded dimension alone, read by those two and nothing else.  The cells come from the column sweeps of
// tools/mb_kernel_param.py and tools/mb_kernel_sm.py (--what wide): a cell is routed to
// k_kinds_mv_wide only where its slowest round beat the one-column kernel's fastest.  From 17 columns on (a second sweep of
// k_kparam_mv / k_ksm_mv) it won in every cell of every family: 0.35 - 0.77 of the time.  At 5 .. 16 columns rational
// quadratic won at DP 16 and 32 (0.68 - 0.78) and lost at DP 4 and 8 (1.03 - 1.09); periodic won at DP 32 only (0.95 -
// 0.96; 1.08 - 1.12 below: its D sines per pair leave the ALU no room beside the matrix cores); spectral mixture won at
// every DP and both Q (0.93 - 0.98).  Up to 4 columns the one-column kernels are kept everywhere, c = 1 included, which
// tests/test_gpu_kernel_variants.py pins by name (the wide kernel won 8 of those 36 cells, rational quadratic at DP 32 by
// 11 - 20 % and spectral mixture by 2 - 11 %, and lost the others by 1 - 97 %).
inline bool kp_wide(int family, int64_t c, int DP) {
  return c >= 17 || (c >= 5 && DP >= (family == LO_KERNEL_PERIODIC ? 32 : 16));
}
inline bool ksm_wide(int64_t c, int DP) { return c >= 5; }

// The layouts of their derivatives' workspaces: a partial per workgroup, [B, rb js, 2 DP + 2] (k_kparam_bil_reduce) and
// [B, Q, rb js, 2 DP + 1] (k_ksm_bil_reduce)
inline float* kp_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * s.rb * s.js * (2 * ko_padded_dim(D) + 2));
}
inline float* ksm_bil_layout(Arena& ar, int64_t B, int64_t M, int64_t N, int64_t D, int64_t Q) {
  const KoShape s = ko_shape(B, M, N);
  return ar.take<float>((size_t)B * Q * s.rb * s.js * (2 * ko_padded_dim(D) + 1));
}
// g_theta from those partials in ascending order, with the factors (lo_kernel_param.hip, lo_kernel_sm.hip)
int kp_bil_reduce(const float* part, int nblk, int DP, int64_t B, int64_t D, int family, const float* theta,
                  float* g_theta, hipStream_t st);
int ksm_bil_reduce(const float* part, int nblk, int DP, int64_t B, int64_t D, int64_t Q, const float* theta,
                   float* g_theta, hipStream_t st);

// Their many-column derivatives with W = U V^T on the matrix cores (lo_kernel_kinds_bil_wide.hip, k_kinds_bil_wide): the
// arguments and the partials of kernel_param_bil_run / kernel_param_pgrad_run / kernel_sm_bil_run / kernel_sm_pgrad_run.
int kernel_param_bil_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                              int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_theta,
                              float* part, hipStream_t st);
int kernel_param_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int family, int64_t B, int64_t M,
                                int64_t N, int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                                hipStream_t st);
int kernel_sm_bil_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                           int64_t D, const float* U, const float* V, int64_t t, float* g_theta, float* part,
                           hipStream_t st);
int kernel_sm_pgrad_wide_run(const float* x1, const float* x2, const float* theta, int Q, int64_t B, int64_t M, int64_t N,
                             int64_t D, const float* U, const float* V, int64_t t, float* g_x1, float* part,
                             hipStream_t st);
// columns of U / V one sweep of those kernels carries, next to ko_bil_wide_cols: half of them per lane in registers for
// each of two rows, beside the lane's point, its running and tile sums and the 32 accumulators of W.  32, but 16 for
// periodic at DP 32, whose hyperparameter kernel (five arrays of 32 and two float64 sums) uses 76 bytes of scratch per
// lane at 32 (DESIGN.md section 6zc holds the table)
constexpr int kp_bil_wide_cols(int family, int DP) { return family == LO_KERNEL_PERIODIC && DP == 32 ? 16 : 32; }
constexpr int ksm_bil_wide_cols(int DP) { return 32; }
// Which of the two those four run functions launch: functions of the family, the column count and the padded dimension
// alone, read by them and nothing else.  The cells come from the derivative sweeps of tools/mb_kernel_param.py and
// tools/mb_kernel_sm.py (--what bilwide): a cell is routed to k_kinds_bil_wide only where its slowest
// round beat the plain kernel's fastest.  From 9 columns on (a second sweep of the plain kernels) it won in every cell of
// every family and both kernels: at 9 .. 16 columns 0.44 - 0.66 of the time (rational quadratic at DP 32: 0.61 - 0.84),
// from 17 on 0.24 - 0.66 (the points of periodic at DP 32, which sweeps 16 columns: 0.65 - 0.86).  Up to 8 columns it won 45
// of the 64 rational-quadratic / periodic cells (0.78 - 0.99) and lost the others (1.00 - 1.55, most of them at DP 32),
// and, of spectral mixture, the points at DP 4 (0.92 - 0.98) but no hyperparameter cell (1.01 - 1.30); those cells keep
// the plain kernels whatever the sweep says: t <= 8 stays on k_kparam_bil / k_kparam_pgrad / k_ksm_bil / k_ksm_pgrad, which
// tests/test_gpu_kernel_variants.py pins by name.
inline bool kp_bil_wide(int family, int64_t t, int DP) { return t >= 9; }
inline bool ksm_bil_wide(int64_t t, int DP) { return t >= 9; }

// y[b, i, col] = sum_z part[z, b, i, col] (ascending z) + d o v over `total` = B rows c elements (lo_kernel_op.hip)
int ko_reduce_splits(const char* prof_name, const float* part, int js, size_t per_member, size_t total, int c,
                     const float* d, int dmode, const float* v, float* y, const int* stop, hipStream_t st);


// g_theta [B, D + 1] from the per-workgroup partials [B, nblk, DP + 1] of a bilinear sweep, in ascending order
// (lo_kernel_op.hip): slot q < D times os2 / theta[q], slot DP (the sum for os2) as it is
int ko_bil_reduce(const float* part, int nblk, int DP, int64_t B, int64_t D, const float* theta, float* g_theta,
                  hipStream_t st);

}  // namespace lo
