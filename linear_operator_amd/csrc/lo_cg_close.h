// lo_cg_close.h -- closing step of the single-column operator-resident solves (k_cg_onchip5, k_cg_rspace, k_cg_rspace3): the
// first workgroup of the group that finishes LAST does what k_cg_ctrl_onchip does (stop rule linear_cg.py:302-308, NaN check
// :199-200, "all converged before the first iteration" :207-208), mirrors the control block to pinned host memory and
// writes the ticket.  Every member left {final residual norm | a.close_epoch + flags} as one 8-byte granule in a.close_gran:
// a granule has arrived when its upper 29 bits are this launch's epoch (0x80000000 over a buffer the host cleared; a
// per-launch value in the library's own block, where the granules of earlier launches stay behind with other epochs).
//
// What a caller has to guarantee (k_cg_rspace3 calls from INSIDE its member loop, in front of its last x pass, so these
// are stated here and argued at that call site; the kernels that call at their very end meet them trivially):
//   (1) a group counts itself in only after its last draw from next_member has returned a value >= B: the closer, the
//       last group to count in, may then reset next_member and close_count for the next launch;
//   (2) the group's last exchange -- the only place a hand-off can be lost -- lies before the count, so the error word
//       the closer mirrors is final (the closer itself may still set it: a granule that never arrives);
//   (3) the state and the close granule of every member of the group were stored (issued) before the count.
// Nothing the closing step reads or writes depends on a member's solution: the host learns from the ticket that `info`
// is final, the solution is complete in stream order (lo_amd.h).
//
// The step lies on the ticket's path, which the host waits for: all of a thread's granule loads of a round are in
// flight together, the four partial values cross the workgroup in ONE pass through LDS, the block is mirrored by one
// lane per word.
#pragma once
#include <cstddef>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_cg_onchip.h"
#include "lo_group_reduce.h"

namespace lo {

// called by the workgroups with wig == 0 (all 256 threads), once per workgroup and launch
__device__ __forceinline__ void cg_close_solve(const OnchipArgs& a, const int ngroups, const int t) {
  constexpr int CW = (int)(sizeof(CgCtrl) / sizeof(int));  // words of the control block: one lane each
  static_assert(sizeof(CgCtrl) == CW * sizeof(int) && CW < 63, "the ticket is word 63 of the pinned block");
  __shared__ int closer_s;
  __shared__ float red_s[R4_WAVES];
  __shared__ unsigned flag_s[R4_WAVES];
  if (t == 0) closer_s = (atomicAdd(a.close_count, 1) == ngroups - 1) ? 1 : 0;
  __syncthreads();
  if (closer_s) {
    // (the other groups' granules were stored before their counter increments, but nothing orders the two for us:
    //  every granule is polled until its tag is there -- no fence anywhere)
    // The words of the block that this step does not own (the hand-out counters, on a caller's workspace): every group
    // has drawn for the last time, they are final.  Requested here, used behind the poll.
    CgCtrl* c = a.close_ctrl;
    unsigned keep = 0u;
    if (t < CW && !a.handoff_owned)
      keep = __hip_atomic_load(reinterpret_cast<const unsigned*>(c) + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The error word, requested with the granules instead of behind the reduction (a dependent round trip to the L2 on
    // the ticket's path): every group's last exchange lies before its count and this group is the last to count, so
    // the word is final from here on -- but for this step's own give-up below, which travels with the flags (8).
    int err0 = 0;
    if (t < 64) err0 = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float lsum = 0.f;
    unsigned lflags = 0u;  // 1: NaN, 2: a member had not converged before the first iteration, 4: redo on the dense form
    unsigned spin = 0;
    bool lost = false;
    constexpr int CK = 4;  // granules of a thread polled together (B = 512: both of them)
    for (int64_t i0 = t; i0 < a.B && !lost; i0 += CK * R4_TPB) {
      unsigned long long gr[CK];
      for (;;) {
        bool ok = true;  // (no short-circuit: all loads of the round are in flight before the first is tested)
#pragma unroll
        for (int q = 0; q < CK; ++q) {
          const int64_t i = i0 + (int64_t)q * R4_TPB;
          gr[q] = granule_load(a.close_gran + (i < a.B ? i : a.B - 1));
          ok = ok && ((granule_tag(gr[q]) & ~7u) == a.close_epoch);
        }
        if (ok) break;
        // DEVIATES from poll_give_up: the error word is read on EVERY miss, and it is set once, after the loop
        if (++spin > kHandoffMaxSpin || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
          lost = true;  // a group gave up (hand-off timeout): its members never arrive -- the host redoes the solve
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      if (lost) break;
#pragma unroll
      for (int q = 0; q < CK; ++q) {  // (ascending members: the order in which a thread has always added them)
        if (i0 + (int64_t)q * R4_TPB < a.B) {
          const float rn = granule_value(gr[q]);
          const unsigned fl = granule_tag(gr[q]);
          lsum += rn;
          if (rn != rn || (fl & 2u)) lflags |= 1u;
          if (!(fl & 1u)) lflags |= 2u;
          if (fl & 4u) lflags |= 4u;  // (diagonal form: this member wants the dense form)
        }
      }
    }
    if (lost) {
      atomicExch(a.err, 1);
      lflags |= 8u;
    }
    // One pass through LDS.  The residual sum keeps the order of block_sum256 / k_cg_ctrl_onchip bit for bit: the xor
    // butterfly 32, 16, .. 1 inside a wave (wave_sum), then (w0 + w1) + (w2 + w3).  The three conditions were sums of
    // 0 / 1 that were only ever compared with zero: a wave's "any" is a ballot, the workgroup's an OR.
    const float wsum = wave_sum(lsum);
    const unsigned wflags = (__ballot(lflags & 1u) ? 1u : 0u) | (__ballot(lflags & 2u) ? 2u : 0u) |
                            (__ballot(lflags & 4u) ? 4u : 0u) | (__ballot(lflags & 8u) ? 8u : 0u);
    if ((t & 63) == 0) {
      red_s[t >> 6] = wsum;
      flag_s[t >> 6] = wflags;
    }
    __syncthreads();
    if (t < 64) {  // (wave 0 as a whole: lane w < CW carries word w of the control block)
      // (opaque copies: formed here.  As loop invariants of a caller's member loop the conversion and the ticket would
      //  each hold a vector register from the kernel's entry on -- k_cg_rspace3 has none to spare)
      long long nb = a.B;
      unsigned ticket = a.close_ticket;
      asm volatile("" : "+s"(nb), "+s"(ticket));
      const float mean = ((red_s[0] + red_s[1]) + (red_s[2] + red_s[3])) / (float)nb;
      const unsigned flags = (flag_s[0] | flag_s[1]) | (flag_s[2] | flag_s[3]);
      // (every field the closing step owns is written: the block need not have been cleared for this launch)
      const bool nan = (flags & 1u) != 0u;
      const bool skip = !nan && !(flags & 2u);     // every column converged before the first iteration (:207-208)
      const bool tol = !nan && !skip && a.close_floor_ok && mean < a.close_tol;
      const int oc_err = (flags & 8u) ? 1 : err0;  // (what a load behind the exchange above would return)
      unsigned w = keep;
      bool mine = a.handoff_owned != 0;  // (owned: err and the counters are not words of *c, its counter words read 0)
      const auto put = [&](size_t off, unsigned v) {
        if ((size_t)t * sizeof(int) == off) {
          w = v;
          mine = true;
        }
      };
      put(offsetof(CgCtrl, rs_redo), (flags & 4u) ? 1u : 0u);
      put(offsetof(CgCtrl, iterations), skip ? 0u : (unsigned)a.iters);
      put(offsetof(CgCtrl, mean_resid), __float_as_uint(mean));
      put(offsetof(CgCtrl, nan_detected), nan ? 1u : 0u);
      put(offsetof(CgCtrl, skipped), skip ? 1u : 0u);
      put(offsetof(CgCtrl, tol_reached), tol ? 1u : 0u);
      put(offsetof(CgCtrl, stop), (nan || skip || tol) ? 1u : 0u);
      put(offsetof(CgCtrl, last_tridiag_iter), 0u);
      put(offsetof(CgCtrl, tri_disabled), 0u);
      put(offsetof(CgCtrl, oc_err), (unsigned)oc_err);
      if (t < CW && mine) reinterpret_cast<unsigned*>(c)[t] = w;
      if (a.handoff_owned && t == 0) {
        // err and the counters are not words of *c here.  Every group has drawn its last member and counted itself in:
        // the next launch (stream order) finds both counters at zero.  err stays as it is: after a lost hand-off the host
        // clears the whole block before it is used again.
        __hip_atomic_store(a.next_member, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.close_count, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (a.close_mirror) {
        if (t < CW) reinterpret_cast<unsigned*>(a.close_mirror)[t] = w;
        // The wave's CW stores are one instruction; the fence is executed by the wave with every lane active (its
        // write-back and its wait for outstanding stores are per wave), then one lane releases the ticket.
        __threadfence_system();
        __builtin_amdgcn_wave_barrier();
        if (t == 0)
          __hip_atomic_store(reinterpret_cast<unsigned*>(a.close_mirror) + 63, ticket, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

}  // namespace lo
