// lo_kernel_task.h -- what the kernels of LO_OP_KERNEL_TASK_DIAG (lo_kernel_task.hip) and its row source in the pivoted
// Cholesky (lo_pivchol.hip) share: how a task id stored as a float becomes an index into Bt.
#pragma once
#include <hip/hip_runtime.h>

namespace lo {

// the id in the last column of a point: rounded to nearest, clamped into [0, T - 1] (NaN reads as 0), so that no id can
// index outside the T x T table
__device__ __forceinline__ int tk_task_id(float f, int T) {
  return (int)rintf(fminf(fmaxf(f, 0.0f), (float)(T - 1)));
}

}  // namespace lo
