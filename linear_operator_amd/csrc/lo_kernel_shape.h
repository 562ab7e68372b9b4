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

// the single-term product on validated arguments (lo_kernel_op.hip); tstride: floats between two members' thetas;
// part: [js, B, M, c] floats when ko_shape(B, M, N).js > 1 (else unused)
int kernel_mv_run(const float* x1, const float* x2, const float* theta, int64_t tstride, int family, int64_t B, int64_t M,
                  int64_t N, int64_t D, const float* v, int64_t c, const float* d, int dmode, float* y, float* part,
                  const int* stop, hipStream_t st);

// y[b, i, col] = sum_z part[z, b, i, col] (ascending z) + d o v over `total` = B rows c elements (lo_kernel_op.hip)
int ko_reduce_splits(const char* prof_name, const float* part, int js, size_t per_member, size_t total, int c,
                     const float* d, int dmode, const float* v, float* y, const int* stop, hipStream_t st);


// g_theta [B, D + 1] from the per-workgroup partials [B, nblk, DP + 1] of a bilinear sweep, in ascending order
// (lo_kernel_op.hip): slot q < D times os2 / theta[q], slot DP (the sum for os2) as it is
int ko_bil_reduce(const float* part, int nblk, int DP, int64_t B, int64_t D, const float* theta, float* g_theta,
                  hipStream_t st);

}  // namespace lo
