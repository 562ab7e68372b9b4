// lo_cg_close.h -- closing step of the single-column operator-resident solves (k_cg_onchip5, k_cg_rspace): the first
// workgroup of the group that finishes LAST does what k_cg_ctrl_onchip does (stop rule linear_cg.py:302-308, NaN check
// :199-200, "all converged before the first iteration" :207-208), mirrors the control block to pinned host memory and
// writes the ticket.  Every member left {final residual norm | a.close_epoch + flags} as one 8-byte granule in a.close_gran:
// a granule has arrived when its upper 29 bits are this launch's epoch (0x80000000 over a buffer the host cleared; a
// per-launch value in the library's own block, where the granules of earlier launches stay behind with other epochs).
#pragma once
#include "lo_device.h"
#include "lo_internal.h"
#include "lo_cg_onchip.h"
#include "lo_group_reduce.h"

namespace lo {

// called by the workgroups with wig == 0 (all 256 threads)
__device__ __forceinline__ void cg_close_solve(const OnchipArgs& a, const int ngroups, const int t) {
  __shared__ int closer_s;
  __shared__ float red_s[R4_TPB];
  if (t == 0) closer_s = (atomicAdd(a.close_count, 1) == ngroups - 1) ? 1 : 0;
  __syncthreads();
  if (closer_s) {
    // (the other groups' granules were stored before their counter increments, but nothing orders the two for us:
    //  every granule is polled until its tag is there -- no fence anywhere)
    float lsum = 0.f, lnan = 0.f, lnotconv = 0.f, lredo = 0.f;
    unsigned spin = 0;
    bool lost = false;
    for (int64_t i = t; i < a.B && !lost; i += R4_TPB) {
      unsigned long long gr;
      for (;;) {
        gr = granule_load(a.close_gran + i);
        if ((granule_tag(gr) & ~7u) == a.close_epoch) break;
        // DEVIATES from poll_give_up: the error word is read on EVERY miss, and it is set once, after the loop
        if (++spin > kHandoffMaxSpin || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          lost = true;  // a group gave up (hand-off timeout): its members never arrive -- the host redoes the solve
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (lost) break;
      const float rn = granule_value(gr);
      const unsigned fl = granule_tag(gr);
      lsum += rn;
      if (rn != rn || (fl & 2u)) lnan = 1.f;
      if (!(fl & 1u)) lnotconv = 1.f;
      if (fl & 4u) lredo = 1.f;  // (diagonal form: this member wants the dense form)
    }
    if (lost) atomicExch(a.err, 1);
    const float mean = block_sum256(lsum, red_s) / (float)a.B;   // (the summation order of k_cg_ctrl_onchip)
    const float anynan = block_sum256(lnan, red_s);
    const float notconv = block_sum256(lnotconv, red_s);
    const float redo = block_sum256(lredo, red_s);
    if (t == 0) {
      CgCtrl* c = a.close_ctrl;
      // (every field the closing step owns is written: the block need not have been cleared for this launch)
      const bool nan = anynan > 0.f;
      const bool skip = !nan && notconv == 0.f;    // every column converged before the first iteration (:207-208)
      const bool tol = !nan && !skip && a.close_floor_ok && mean < a.close_tol;
      c->rs_redo = redo > 0.f ? 1 : 0;
      c->iterations = skip ? 0 : a.iters;
      c->mean_resid = mean;
      c->nan_detected = nan ? 1 : 0;
      c->skipped = skip ? 1 : 0;
      c->tol_reached = tol ? 1 : 0;
      c->stop = (nan || skip || tol) ? 1 : 0;
      c->last_tridiag_iter = 0;
      c->tri_disabled = 0;
      c->oc_err = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.handoff_owned) {
        // err and the counters are not words of *c here.  Every group has drawn its last member and counted itself in:
        // the next launch (stream order) finds both counters at zero.  err stays as it is: after a lost hand-off the host
        // clears the whole block before it is used again.
        c->oc_next = c->oc_next_ls = c->pf_next = 0;
        __hip_atomic_store(a.next_member, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.close_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (a.close_mirror) {
        *a.close_mirror = *c;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned*>(a.close_mirror) + 63, a.close_ticket, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

}  // namespace lo
