// lo_kernel_tile.h -- what the sweeps of the matrix-free kernel family share on the device (lo_kernel_op.hip,
// lo_kernel_op_f64.hip, lo_kernel_param.hip).  Plain inlined functions: a kernel that uses one compiles to the
// instructions it had with the text written out (profiles/r19 holds the comparison, and the helpers that did not pass it).
#pragma once
#include "lo_internal.h"

namespace lo {

// stage the tile [jt, jt + nj) of x2, scaled coordinate by coordinate by sc, as xs[j][DP] (coordinates >= D are 0)
template <int DP, class T>
__device__ __forceinline__ void ko_stage_points(const T* __restrict__ x2b, const T* __restrict__ sc, int D, int jt, int nj,
                                                T* __restrict__ xs) {
  for (int e = threadIdx.x; e < nj * DP; e += kThreads) {
    const int j = e / DP, dd = e - j * DP;
    xs[e] = dd < D ? x2b[(size_t)(jt + j) * D + dd] * sc[dd] : T(0);
  }
}

// a compensated (Kahan) running sum: the one-number-per-member entries of the derivatives, N M terms of both signs
struct KoKahan {
  float s = 0.0f, c = 0.0f;
  __device__ __forceinline__ void add(float w, float x) {
    const float term = fmaf(w, x, -c);
    const float next = s + term;
    c = (next - s) - term;
    s = next;
  }
};

}  // namespace lo
