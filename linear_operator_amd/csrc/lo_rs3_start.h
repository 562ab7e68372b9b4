// lo_rs3_start.h -- the ordered start of k_cg_rspace3 (lo_rspace3.hip): how long the workgroups of a group
// hold back the first request of the group's FIRST member, so that the groups that share compute units do not load,
// reduce and sit in their iteration chains in phase.  Pure integer functions of the launch's shape, the same on the host
// (rspace3_go forms the kernel argument, lo_resident_start_delay evaluates the rule without a device) and in the kernel
// (every workgroup forms its group's wait from the argument, in scalar registers).
//
// Ticks are those of wall_clock64(): 100 MHz, 10 ns.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace lo {

constexpr int R3_START_CAP_TICKS = 800;      // no workgroup ever waits longer: 8 us
constexpr int R3_START_MIN_ROUNDS = 6;       // a launch of fewer rounds starts at once: the groups stay out of phase round
                                             // after round, so what a wait buys grows with the rounds while its price does
                                             // not -- below six rounds the gain was inside the noise or negative
constexpr int R3_START_DELTA_TICKS = 200;    // the committed delta: 2 us a step
constexpr int R3_START_MAX_STEPS = 3;        // the automatic rule holds only where no group waits more steps than this
                                             // (6 us): the layouts it was measured in (profiles/r14/sweep.txt)

// modes of lo_resident_start_debug (HandoffBlock::start_mode)
enum : int {
  R3_START_AUTO = 0,   // the committed rule: r3_start_auto_delta
  R3_START_OFF = 1,    // never
  R3_START_ON = 2,     // the committed delta whatever the rounds and the layout
  R3_START_GIVEN = 3   // a given delta
};

// The pattern.  The dispatcher hands an XCD its workgroups in order and fills the first slot of every CU before the
// second: the lower half of the XCD's groups (local index li < half) enters together, the upper half -- the second
// workgroup of the same CUs -- about 4 us later (profiles/r14/stamps.txt).  The start is ordered inside each of these
// two dispatch waves: a group waits (its index inside its wave) steps of delta.
__host__ __device__ inline int r3_start_steps(int li, int groups_per_xcd) {
  const int half = groups_per_xcd > 1 ? groups_per_xcd / 2 : 1;
  return li >= half ? li - half : li;
}

// The committed delta of a launch of `rounds` rounds (members / groups, rounded up) in groups_per_xcd groups per XCD:
// nothing in short launches, and nothing in layouts whose waves are longer than the ones the rule was measured in
// (groups of 1, 2 or 4 workgroups on a whole device: 32, 16 or 8 groups a wave -- most of them would sit at the cap
// and then start together).
__host__ __device__ inline int r3_start_auto_delta(int64_t rounds, int groups_per_xcd) {
  if (rounds < R3_START_MIN_ROUNDS || groups_per_xcd <= 0) return 0;
  if (r3_start_steps(groups_per_xcd - 1, groups_per_xcd) > R3_START_MAX_STEPS) return 0;  // (the last group waits longest)
  return R3_START_DELTA_TICKS;
}

// The kernel argument (OnchipArgs::start_delay): delta in ticks, 0 = no wait anywhere.
__host__ __device__ inline int r3_start_arg(int mode, int delta_ticks, int64_t B, int ngroups) {
  if (mode == R3_START_OFF || ngroups <= 0) return 0;
  const int delta = mode == R3_START_AUTO ? r3_start_auto_delta((B + ngroups - 1) / ngroups, ngroups / 8)
                    : mode == R3_START_ON ? R3_START_DELTA_TICKS : delta_ticks;
  return delta < 0 ? 0 : (delta > R3_START_CAP_TICKS ? R3_START_CAP_TICKS : delta);
}

// Ticks the group of local index `li` waits (the kernel has li without a division).  The same for every workgroup of a
// group -- a stagger inside a group would be skew at its first exchange -- and capped whatever the argument holds.
__host__ __device__ inline int r3_start_delay_local(int arg, int li, int groups_per_xcd) {
  const int delta = arg < 0 ? 0 : (arg > R3_START_CAP_TICKS ? R3_START_CAP_TICKS : arg);
  const int d = r3_start_steps(li, groups_per_xcd) * delta;
  return d > R3_START_CAP_TICKS ? R3_START_CAP_TICKS : d;
}
// Ticks group `grp` of the launch waits: groups are numbered XCD by XCD (group_place: grp = xcd * groups_per_xcd + li).
__host__ __device__ inline int r3_start_delay(int arg, int grp, int groups_per_xcd) {
  if (groups_per_xcd <= 0) return 0;
  return r3_start_delay_local(arg, grp % groups_per_xcd, groups_per_xcd);
}

}  // namespace lo
