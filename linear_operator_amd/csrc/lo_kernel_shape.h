// lo_kernel_shape.h -- what the single-term kernels (lo_kernel_op.hip) and the fused multi-term kernels
// (lo_kernel_sum.hip) of the matrix-free kernel operator share: argument checks, the launch shape, the padded sizes and
// the reduction of the column splits.
#pragma once
#include <algorithm>

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
