// lo_rspace3.hip -- k_cg_rspace<.., true> (lo_rspace.hip: the preconditioned CG of a low-rank + diagonal member as the CG of a
// DIAGONAL matrix on its R + 1 Krylov coordinates, linear_operator/utils/linear_cg.py:245-332) in the register layout of the
// one-pass matvec (lo_lowrank_mv.hip).  Same algebra, same iteration chain (copied operation for operation), same outputs;
// what changed is everything around the chain, which is where a member spent 14 of its 20 us:
//
//   * NO transposition window: lane (g = l / CH, k = l % CH) keeps the 16-byte chunk k of the rows RPI i + g of its wave's
//     256 rows -- every wave load is 1 KiB of consecutive addresses and the registers are used as they arrive.  The old
//     layout (a row per lane) moved every row set through a 32 KB LDS window: 4 x (8 ds_write_b128 + 8 ds_read_b128) per lane
//     and two wave barriers per row set on the critical path of the member load (6.4 - 10 us; here 3 - 4.5 us);
//   * the reduction over the rows (w0 = C^T D^-1 b, u0 = C^T b, fp64) accumulates the lane's chunk over its 32 rows (8
//     accumulators instead of 2 x 8 per 8-column block), the right-hand side and 1/d come from a per-wave LDS stage as
//     broadcast reads; ONE reduce-scatter of 8 values over the lanes that share a chunk leaves the 64 totals of the wave
//     in its 64 lanes (the old layout: four 16-value reduce-scatters);
//   * three of the form's matrices in LDS (TinT | TuT | G2: 26 KB instead of four in 35 KB), no 32 KB window: 45 KB per
//     workgroup; the group all-reduce polls with every thread (granule pairs spread over the 256 threads, all loads of a
//     thread in flight together) instead of 2 GW loads in each of 68 threads; the placement check rides on the group's
//     first exchange;
//   * x = D^-1 (xi b + C (nrm y)) in fp64 from the same registers: row sums reduce-scattered over the CH lanes of a row, a
//     wave store covers 64 consecutive rows;
//   * (second pass) a member starts with all of its rows already requested: a quarter during the previous member's
//     iterations, the rest inside its x pass (168 -> 152 us per launch on one box, 142.5 us in the committed profile);
//   * (third pass, profiles/r12) work the result does not need is off the member's serial path: the last iteration's
//     residual norm is formed by workgroup 0 only and, but for a group's final member, at the NEXT member's top while
//     its loads travel; the member draw no longer waits for its own round trip in front of the top's requests; one
//     poll round per exchange up to 9 granules a thread; the exit product's LDS reads are in flight together
//     (143.6 -> 139.9 us per launch);
//   * (fourth pass, profiles/r13) consecutive solves of one operator walk the members in opposite directions
//     (OnchipArgs::member_flip, decided in rspace3_go): a solve starts with the members the previous one left in the
//     256 MiB memory-side cache instead of the ones it evicted first (139.2 -> 131.1 us per launch);
//   * (fifth pass, profiles/r14) the ordered start: in a launch of six rounds or more the groups that the dispatcher
//     starts together wait 0, 1, 2, 3 steps of a delay at the kernel's entry (OnchipArgs::start_delay, lo_rs3_start.h)
//     and stay out of phase from then on (132.9 -> 129.9 us per launch in the tool's timing).
//
// Numerics: fp64 sums in another order (the old kernel's results to ~1e-15 relative before the final rounding to fp32).
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <stdlib.h>

#include "lo_device.h"
#include "lo_internal.h"
#include "lo_cg_onchip.h"
#include "lo_group_reduce.h"
#include "lo_cg_close.h"
#include "lo_f64_lanes.h"
#include "lo_rs3_start.h"

namespace lo {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const f32x4 g_cf4;
typedef __attribute__((address_space(1))) const float g_cf;
typedef __attribute__((address_space(1))) float g_f;
typedef __attribute__((address_space(1))) const char g_cc;
template <class T>
__device__ __forceinline__ T* opaque_uniform(T* p) {
  asm volatile("" : "+s"(p));
  return p;
}

constexpr int R3_TPB = 256;
constexpr int R3_ROWS = 1024;

// Gather by peer writes (prototype, SURVEY 8(e): "one RCCL all-gather over xGMI at the end"): the x pass can store every
// solution value into up to seven more buffers next to the caller's -- on a node these would be the IPC-mapped gather
// buffers of the seven peers (each rank writes its slice straight over its own xGMI link while the solve runs; no RCCL
// kernel competes for CUs with the spin-waiting groups).  lo_peer_gather_set installs the pointers for the calling
// process; tools/mb_peer_gather.py emulates the peers with local buffers and times the solve with and without them.
struct PeerOut {
  float* buf[7];
  int n;
  long long member_off;  // this rank's first member inside a peer's gather buffer
};
PeerOut g_peer_out = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, 0, 0};
std::mutex g_peer_mu;  // lo_peer_gather_set against the snapshot a launch takes

__host__ __device__ constexpr int r3_np(int RC) { return 2 * RC + 6; }  // w0 | u0 | s | a0 | next member | sum dinv^2 | xcc | xcc^2

// xor-4 exchange of a double on the DPP path (xor4_dpp_i, lo_device.h, per word)
__device__ __forceinline__ unsigned xor4_dpp_u(unsigned x) { return (unsigned)xor4_dpp_i((int)x); }
__device__ __forceinline__ double halve4_d(double lo, double hi, int lane) {
  const bool up = (lane & 4) != 0;
  const double keep = up ? hi : lo;
  const double send = up ? lo : hi;
  return keep + mk_d(xor4_dpp_u(lo_w(send)), xor4_dpp_u(hi_w(send)));
}

// sum of one row's CH lane partials for CH rows at once (fp64): lane k ends with the total of p[k]
template <int CH>
__device__ __forceinline__ double rows_reduce_d(double (&p)[CH], int lane) {
  if constexpr (CH == 8) {
#pragma unroll
    for (int m = 0; m < 4; ++m) p[m] = halve4_d(p[m], p[m + 4], lane);
    p[0] = halve_pair_d<2>(p[0], p[2], lane);
    p[1] = halve_pair_d<2>(p[1], p[3], lane);
    return halve_pair_d<1>(p[0], p[1], lane);
  } else if constexpr (CH == 4) {
    p[0] = halve_pair_d<2>(p[0], p[2], lane);
    p[1] = halve_pair_d<2>(p[1], p[3], lane);
    return halve_pair_d<1>(p[0], p[1], lane);
  } else {
    return halve_pair_d<1>(p[0], p[1], lane);
  }
}

// ---- pieces of the iteration chain that the member loop uses at two places (the chain, and the next member's top) ----
__device__ __forceinline__ double pick_d(double v, int ln_) {
  return mk_d((unsigned)__builtin_amdgcn_readlane((int)lo_w(v), ln_), (unsigned)__builtin_amdgcn_readlane((int)hi_w(v), ln_));
}
// (M v)_j for the lane pair (j, j + 32): each half-wave takes NH columns of row j, the halves are added lower + upper
template <int NH>
__device__ __forceinline__ double own_row_dot(const double* mrow, const double* vec) {
  double a0_ = 0.0, a1_ = 0.0;
#pragma unroll
  for (int q = 0; q < NH; q += 2) {
    const double2 xa = *reinterpret_cast<const double2*>(mrow + q);
    const double2 xx = *reinterpret_cast<const double2*>(vec + q);
    a0_ = fma(xa.x, xx.x, a0_);
    a1_ = fma(xa.y, xx.y, a1_);
  }
  double lo_, up_;
  halves_d(a0_ + a1_, lo_, up_);
  return lo_ + up_;
}
// Residual norm in the coordinates of C, as the dense form: r = c' r0 + C g with g = Tu del, del = c - c' c0, and
// r^T r = c'^2 a0 + 2 c' g.u0 + g^T G2 g.  `vec` is a 32-double LDS vector of the calling wave (overwritten); tucol is
// this half's part of column j of TuT, nrow this half's part of row j of G2.
template <int NH, int MLD>
__device__ __forceinline__ float resid_norm_c(double dl, double cp, double a0, double u0, bool live, int j, int hf, int lane,
                                              double* vec, const double* tucol, const double* nrow) {
  __builtin_amdgcn_wave_barrier();
  if (hf == 0) vec[j] = dl;
  __builtin_amdgcn_wave_barrier();
  double gj_;
  {
    double a0_ = 0.0, a1_ = 0.0;
#pragma unroll
    for (int q = 0; q < NH; q += 2) {
      const double2 dd = *reinterpret_cast<const double2*>(vec + hf * NH + q);
      a0_ = fma(tucol[(size_t)q * MLD], dd.x, a0_);
      a1_ = fma(tucol[(size_t)(q + 1) * MLD], dd.y, a1_);
    }
    double lo_, up_;
    halves_d(a0_ + a1_, lo_, up_);
    gj_ = live ? lo_ + up_ : 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  if (hf == 0) vec[j] = gj_;
  __builtin_amdgcn_wave_barrier();
  const double nd = own_row_dot<NH>(nrow, vec + hf * NH);      // (G2 g)_j
  const double r2 = row16_sum_d(halve_pair_d<16>(gj_ * nd, gj_ * u0, lane));
  const double dnd = pick_d(r2, 0), dm = pick_d(r2, 16);
  const double s1 = fma(cp, fma(cp, a0, 2.0 * dm), dnd);       // r^T r
  const float s1f = (float)s1;
  return __builtin_amdgcn_sqrtf(s1f < 0.f ? 0.f : s1f);
}

template <int RC, int GW>
__global__ __launch_bounds__(R3_TPB, 2) void k_cg_rspace3(OnchipArgs a, PeerOut po) {
  constexpr int CH = RC / 4;     // 16-byte chunks per row
  constexpr int RPI = 64 / CH;   // rows per wave load instruction
  constexpr int NI = 256 / RPI;  // load instructions per wave
  constexpr int NP = r3_np(RC);
  constexpr int MLD = RC + 2;    // row stride of the fp64 matrices in LDS (16-byte aligned, conflict-free b128 reads)
  constexpr int NH = RC / 2;     // columns per half-wave in the R x R products
  constexpr int NG = 2 * GW * NP;  // granules of one exchange (two per double)
  __shared__ __attribute__((aligned(16))) float bst[4][256];   // right-hand side of the wave's rows
  __shared__ __attribute__((aligned(16))) float dst[4][256];   // 1 / d of the wave's rows
  __shared__ __attribute__((aligned(16))) double mat_s[3 * RC * MLD];  // TinT | TuT | G2
  __shared__ __attribute__((aligned(16))) double red[4][NP];
  __shared__ __attribute__((aligned(16))) double res[NP];
  __shared__ __attribute__((aligned(16))) double gv[4][32];
  __shared__ unsigned polw[GW > 1 ? NG : 2];
  // what the last residual norm of a member needs when it is formed at the next member's top (below): del | c' | close
  // flags | member.  Its own vector: gv[wave] holds nrm * y for the x pass by then.
  __shared__ __attribute__((aligned(16))) double late_v[32 + 4];
  const GroupPlace gp = group_place(GW, (int)gridDim.x / 8);
  if (!gp.active) return;  // (surplus workgroup)
  // The ordered start (lo_rs3_start.h): a group's FIRST member asks for its rows start_delay(group) ticks behind this
  // wave's entry -- the same wait in every workgroup of the group -- so that the groups the dispatcher starts
  // together do not load, reduce and iterate in phase.  The wait reads the clock and nothing else, ends at the cap
  // whatever the argument holds, and stands here, in front of everything the member loop keeps in registers: scalar
  // registers only, from opaque copies (behind the first request it cost a vector-register spill at 32 columns).  A
  // group without a member (grp >= B) never waits; no later member does.
  {
    int sd = a.start_delay, g0 = gp.grp, li = (int)(blockIdx.x / 8) / GW;  // (li: the group's local index inside its XCD)
    asm volatile("" : "+s"(sd), "+s"(g0), "+s"(li));
    const unsigned wait = (sd != 0 && g0 < a.B) ? (unsigned)r3_start_delay_local(sd, li, (int)gridDim.x / 8 / GW) : 0u;
    if (wait > 0) {  // (<= R3_START_CAP_TICKS)
      const unsigned t_in = (unsigned)wall_clock64();  // (low words: the differences below are exact modulo 2^32)
#pragma unroll 1
      for (int n = 0; n < 4 * R3_START_CAP_TICKS && (unsigned)wall_clock64() - t_in < wait; ++n)
        __builtin_amdgcn_s_sleep(1);
    }
  }
  const int grp = gp.grp, wig = gp.wig, ngroups = gp.ngroups;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  unsigned long long* const gbase = a.gbuf + (size_t)grp * 2 * NG;  // [parity][GW][NP][2]
  unsigned tag = a.tag_base;  // (0 over a cleared buffer; above every earlier launch's tags in the library's own block)
  bool same_xcd = false;
  const unsigned xcc = xcc_id();
  bool first = true;
  // rows: a wave owns [row0, row0 + 256); it loads from row0c = min(row0, N - 256) on (no per-row clamp: lo_lowrank_mv.hip),
  // rows below row0 belong to the previous wave and enter with b = 0 and 1/d = 0, as do rows >= N
  const int row0 = wig * R3_ROWS + 256 * wave_u;
  const int row0c = max(0, min(row0, a.N - 256));
  const bool di_full = a.dinv_mode == LO_DIAG_FULL;
  float* const bw = bst[wave_u];
  float* const dw = dst[wave_u];
  // The first NPF load instructions of a member's rows (a QUARTER of them at 32 columns: half spills) are
  // requested while the PREVIOUS member's iterations run: the registers the chain leaves free hold them (C of the current
  // member stays for its x pass) and the requests travel while this workgroup would otherwise ask HBM for nothing.  The
  // other instructions (nxt[]) are requested inside the previous member's x pass, group by group as it frees their
  // registers.  Both arrays are carried around the member loop; the first member's rows are requested here.
  constexpr int NPF = 8;  // (a quarter of the rows at 32 columns, half at 16, all at 8)
  f32x4 pre[NPF];
  constexpr int NXT = NI - NPF;          // the other load instructions: requested while the x pass frees their registers
  f32x4 nxt[NXT > 0 ? NXT : 1];
  auto request = [&](int64_t bm, int tl_, int i_lo, auto cnt, f32x4* dst) {  // load instructions i_lo .. i_lo + cnt - 1 of member bm
    const int ln_ = tl_ & 63, k_ = ln_ & (CH - 1), g_ = ln_ / CH;
    const unsigned loff = (unsigned)((g_ * RC + 4 * k_) * sizeof(float));
    g_cc* Cw = (g_cc*)(a.C + ((size_t)bm * a.N + row0c) * RC);
#pragma unroll
    for (int q = 0; q < decltype(cnt)::value / 8; ++q) {
      g_cc* bq = opaque_uniform(Cw + (i_lo + 8 * q + 4) * 1024);
#pragma unroll
      for (int i = 0; i < 8; ++i) dst[8 * q + i] = *(g_cf4*)(bq + loff + (i - 4) * 1024);
    }
  };
  int closed = 0;  // workgroup-uniform: this workgroup has run the closing step (inside the loop, below)
  bool late_pending = false;  // workgroup-uniform: the previous member's last residual norm is still to be formed
  // Members are DRAWN by logical index b (grp first, then ngroups + the hand-out counter, as ever) and ADDRESSED by the
  // physical index m = flip ? B - 1 - b : b: a launch that follows one on the same operator walks the batch the other way
  // round and finds the members the previous launch read last still in the memory-side cache (rspace3_go).
  // Everything a member owns in memory -- operator, right-hand side, matrices, x, records, close granule -- goes by m; a
  // member's arithmetic does not depend on when it runs, so results are the same bit for bit in either direction.
  const bool flip = a.member_flip != 0;
  // (debug stamps: the launch's origin on the time axis of the stamped member -- group 0 enters with the first wave of
  //  workgroups; kept in memory, not in a register around the member loop)
  if (a.dbg && grp == 0 && wig == 0 && t == 0) a.dbg[11] = wall_clock64();
  int64_t b = grp;
  {
    int tl0 = t;
    asm volatile("" : "+v"(tl0));
    if (b < a.B) {
      const int64_t m0 = flip ? a.B - 1 - b : b;
      request(m0, tl0, 0, std::integral_constant<int, NPF>{}, pre);
      request(m0, tl0, NPF, std::integral_constant<int, NXT>{}, nxt);
    } else {
#pragma unroll
      for (int i = 0; i < NPF; ++i) pre[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  while (b < a.B) {
    const int64_t m = flip ? a.B - 1 - b : b;  // (workgroup-uniform: scalar registers only)
    const bool stamp = a.dbg && m == a.dbg_member && wig == 0 && t == 0;
    if (stamp) a.dbg[0] = wall_clock64();
    int drawn = 0;
    // (its round trip hides behind the member load -- through a pointer whose address space the compiler cannot see: on a
    //  global pointer the wave-level combining of atomics reads the result back with v_readfirstlane right here, behind
    //  an s_waitcnt vmcnt(0) that also waits for every row still in flight, and the requests below start only then)
    if (wig == 0 && t == 0) drawn = atomicAdd(opaque_uniform(a.next_member), 1);
    int tl = t;
    asm volatile("" : "+v"(tl));
    const int ln = tl & 63, k = ln & (CH - 1), g = ln / CH;
    // ---- every request of the member in flight before anything waits ----
    f32x4 Cr[NI];
#pragma unroll
    for (int i = 0; i < NPF; ++i) Cr[i] = pre[i];   // (requested during the previous member's iterations)
#pragma unroll
    for (int i = 0; i < NXT; ++i) Cr[NPF + i] = nxt[i];
    float bq4[4], dq4[4];
    {
      g_cf* bb_ = opaque_uniform((g_cf*)(a.rhs + (size_t)m * a.N + row0c));
      g_cf* dd_ = opaque_uniform((g_cf*)(di_full ? a.dinv + (size_t)m * a.N + row0c : a.dinv + m));
      const int lo_e = row0 - row0c, hi_e = max(0, min(256, a.N - row0c));
      const int dstride = di_full ? 1 : 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int e = ln + 64 * m;
        const bool own = e >= lo_e && e < hi_e;
        bq4[m] = own ? bb_[e] : 0.f;
        dq4[m] = own ? dd_[e * dstride] : 0.f;
      }
    }
    // TinT | TuT | G2 of the diagonal form (matrices 0, 2, 3 of lo_precond_desc.RSD), 16-byte pieces
    constexpr int NM = (3 * RC * RC / 2 + R3_TPB - 1) / R3_TPB;
    f32x4 mv[NM];
    {
      typedef __attribute__((address_space(1))) const f32x4 g_m4;
      const g_m4* src = (const g_m4*)(a.RSD + (size_t)m * 6 * RC * RC);
#pragma unroll
      for (int u = 0; u < NM; ++u) {
        const int e = min(tl + R3_TPB * u, 3 * RC * RC / 2 - 1);  // piece e of the three matrices in LDS order
        const int ms = e / (RC * RC / 2);                        // 0, 1, 2 -> matrix 0, 2, 3
        const int mg = ms == 0 ? 0 : ms + 1;
        mv[u] = src[(size_t)mg * (RC * RC / 2) + (e - ms * (RC * RC / 2))];
      }
    }
    const double lam_mine = a.RSD[((size_t)m * 6 + 5) * RC * RC + min(ln & 31, RC - 1)];  // this lane's eigenvalue
    // ---- the last residual norm of the PREVIOUS member, when that was not the group's final one (see `late` below) ----
    // Every request of this member is in flight and nothing has arrived: the wave that owes the norm forms it here, from
    // what it left in late_v, while all four waves wait for their loads anyway.  mat_s (TuT, G2) and res[] are still the
    // previous member's: the barrier that releases them to this member stands BEHIND this block, not at the end of the
    // previous member's x pass (between the two places nothing touches LDS that another wave reads: the stages bst / dst
    // and gv are per wave).  u0, a0 and nrm are formed from res[] as the chain's entry forms them.  The records and the
    // close granule leave in front of the barrier, so the closing step of the group's final member -- behind at least
    // this barrier -- finds them issued (lo_cg_close.h (3)).
    if (late_pending && wave_u == ((a.iters - 1) & 3)) {
      int l3 = lane;
      asm volatile("" : "+v"(l3));
      const int j = l3 & 31, hf = l3 >> 5;
      const bool live = j < RC;
      const int jr = live ? j : RC - 1;
      double a0 = res[2 * RC + 1];
      float nrm = sqrtf((float)a0);
      const bool rhs_zero = nrm < a.eps;
      if (rhs_zero) nrm = 1.0f;
      const double inv = 1.0 / (double)nrm;
      const double u0 = live ? res[RC + jr] * inv : 0.0;
      a0 *= inv * inv;
      const double* tucol = mat_s + (size_t)(1 * RC + hf * NH) * MLD + jr;
      const double* nrow = mat_s + (size_t)(2 * RC + jr) * MLD + hf * NH;
      const double dl = late_v[j], cp = late_v[32];
      const unsigned flags0 = (unsigned)late_v[33];
      const size_t bp = (size_t)late_v[34];  // the previous member (exact: members are counted in fp64 by the exchange too)
      float rn = resid_norm_c<NH, MLD>(dl, cp, a0, u0, live, j, hf, l3, late_v, tucol, nrow);
      if (rhs_zero) rn = 0.f;
      if (l3 == 0) {
        // (opaque copies: formed here.  As invariants of the member loop the record's offset is kept in vector registers
        //  from the kernel's entry on, and spilled)
        int it = a.iters;
        long long nb = a.B;
        asm volatile("" : "+s"(it), "+s"(nb));
        const unsigned close_flags = flags0 | ((it == 1 && rn != rn) ? 2u : 0u);  // (NaN after the first product)
        a.resid_rec[(size_t)(it - 1) * (size_t)nb + bp] = rn;
        a.resid_norm[bp] = rn;
        a.has_conv[bp] = (rn < a.stop_after) ? 1 : 0;
        if (a.close_gran) {
          granule_store(a.close_gran + bp, granule_pack(a.close_epoch | close_flags, rn), /*same_xcd=*/false);
        }
      }
    }
    __syncthreads();  // the previous member's matrices and res[] may be replaced from here on
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      bw[ln + 64 * m] = bq4[m];
      dw[ln + 64 * m] = dq4[m];
    }
#pragma unroll
    for (int u = 0; u < NM; ++u) {
      const int e = tl + R3_TPB * u;
      if (e < 3 * RC * RC / 2) {
        const int mi = e / (RC / 2), jj = e % (RC / 2);  // (matrix slot * RC + row, column pair)
        *reinterpret_cast<f32x4*>(&mat_s[mi * MLD + 2 * jj]) = mv[u];
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (stamp) a.dbg[1] = wall_clock64();

    // ---- the member's one reduction over the rows, fp64: w0 = C^T (dinv o b), u0 = C^T b (this lane's chunk), s, a0 ----
    {
      double aw[4] = {0.0, 0.0, 0.0, 0.0}, au[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i0 = 0; i0 < NI; i0 += 4) {
#pragma unroll
        for (int i = i0; i < i0 + 4; ++i) {
          const int r = RPI * i + g;
          const double bb = (double)bw[r];
          const double bd = bb * (double)dw[r];
          const double c0 = (double)Cr[i].x, c1 = (double)Cr[i].y, c2 = (double)Cr[i].z, c3 = (double)Cr[i].w;
          aw[0] = fma(c0, bd, aw[0]); au[0] = fma(c0, bb, au[0]);
          aw[1] = fma(c1, bd, aw[1]); au[1] = fma(c1, bb, au[1]);
          aw[2] = fma(c2, bd, aw[2]); au[2] = fma(c2, bb, au[2]);
          aw[3] = fma(c3, bd, aw[3]); au[3] = fma(c3, bb, au[3]);
        }
        // (four rows at a time: the scheduler otherwise hoists all 64 stage reads and their conversions over the loop and
        //  spills 36 registers of C around the reduction)
        __builtin_amdgcn_sched_barrier(0);
      }
      // scalars over the lane's own four rows 64 j + RPI k + g (every row of the wave exactly once)
      double s_acc = 0.0, a_acc = 0.0, d2_acc = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int rw = 64 * j + RPI * k + g;
        const double bb = (double)bw[rw], di = (double)dw[rw];
        s_acc = fma(bb, bb * di, s_acc);
        a_acc = fma(bb, bb, a_acc);
        d2_acc = fma(di, di, d2_acc);
      }
      // reduce-scatter over the lanes that share a chunk: bit 5 -> w0 | u0, bits 4, 3 -> component of the chunk
      double h0 = halve_pair_d<32>(aw[0], au[0], ln), h1 = halve_pair_d<32>(aw[1], au[1], ln);
      double h2 = halve_pair_d<32>(aw[2], au[2], ln), h3 = halve_pair_d<32>(aw[3], au[3], ln);
      h0 = halve_pair_d<16>(h0, h2, ln);
      h1 = halve_pair_d<16>(h1, h3, ln);
      double mine = halve_pair_d<8>(h0, h1, ln);
      if constexpr (CH <= 4) mine = bfly_add_d<4>(mine);
      if constexpr (CH <= 2) mine = bfly_add_d<2>(mine);
      const int comp = (((ln >> 4) & 1) << 1) | ((ln >> 3) & 1);
      const bool writer = (ln & 7 & ~(CH - 1)) == 0;
      if (writer) red[wave_u][((ln >> 5) ? RC : 0) + 4 * k + comp] = mine;
      const double ssum = wave_sum_fast_d(s_acc), asum = wave_sum_fast_d(a_acc), d2sum = wave_sum_fast_d(d2_acc);
      if (ln == 0) {
        red[wave_u][2 * RC] = ssum;
        red[wave_u][2 * RC + 1] = asum;
        red[wave_u][2 * RC + 2] = (wig == 0 && wave_u == 0) ? (double)(ngroups + drawn) : 0.0;
        red[wave_u][2 * RC + 3] = d2sum;
        // (loop invariants that are cheaper to form than to keep: opaque copies, or they are spilled around the loop and
        //  their reload waits behind every request in flight)
        unsigned xc = xcc;
        asm volatile("" : "+s"(xc));
        red[wave_u][2 * RC + 4] = (first && wave_u == 0) ? (double)xc : 0.0;
        red[wave_u][2 * RC + 5] = (first && wave_u == 0) ? (double)(xc * xc) : 0.0;
      }
    }
    // (opaque to value numbering: otherwise the fp64 conversions of the rows are kept -- and spilled -- for the last pass)
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(Cr[i]));
    __builtin_amdgcn_sched_barrier(0);
    // ---- group all-reduce of NP doubles (two tagged granules each): the first NP threads publish, ALL threads poll ----
    if (a.prefetch & 4) __builtin_amdgcn_s_setprio(3);
    {
      ++tag;
      int tt = (int)threadIdx.x;
      asm volatile("" : "+v"(tt));
      __syncthreads();
      if constexpr (GW == 1) {
        if (tt < NP) res[tt] = (red[0][tt] + red[1][tt]) + (red[2][tt] + red[3][tt]);
      } else {
        unsigned long long* slot = gbase + (size_t)(tag & 1u) * NG;
        if (tt < NP) {
          const double v = (red[0][tt] + red[1][tt]) + (red[2][tt] + red[3][tt]);
          unsigned long long* mine = slot + ((size_t)wig * NP + tt) * 2;
          granule_store(mine, granule_pack_bits(tag, lo_w(v)), same_xcd);
          granule_store(mine + 1, granule_pack_bits(tag, hi_w(v)), same_xcd);
        }
        constexpr int PER = (NG + R3_TPB - 1) / R3_TPB;  // granules per thread
        // ... polled together: all of them up to 9 (<32, 8>: ONE round of 9, where a round of 8 was followed by a dependent
        // round for one granule and seven clamped duplicates), two equal rounds up to 18 (<32, 16>: 9 + 9), rounds of 8
        // in groups of 32 workgroups
        constexpr int CKQ = GW == 32 ? 8 : PER <= 9 ? PER : (PER + 1) / 2;
        static_assert(CKQ <= 9 && 2 * CKQ >= (GW == 32 ? 16 : PER), "poll rounds");
        unsigned spin = 0;
        bool lost = false;
#pragma unroll 1
        for (int q0 = 0; q0 < PER && !lost; q0 += CKQ) {
          unsigned long long x[CKQ];
          for (;;) {
            bool ok = true;
#pragma unroll
            for (int q = 0; q < CKQ; ++q) {
              const int idx = tt + R3_TPB * (q0 + q);
              x[q] = granule_load(slot + min(idx, NG - 1));
              ok = ok && (granule_tag(x[q]) == tag);
            }
            if (ok) break;
            if (poll_give_up(spin, a.err)) {
              lost = true;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
#pragma unroll
          for (int q = 0; q < CKQ; ++q) {
            const int idx = tt + R3_TPB * (q0 + q);
            if (idx < NG) polw[idx] = granule_bits(x[q]);
          }
        }
        __syncthreads();
        if (tt < NP) {
          double tot = 0.0;
#pragma unroll
          for (int w = 0; w < GW; ++w) tot += mk_d(polw[(w * NP + tt) * 2], polw[(w * NP + tt) * 2 + 1]);  // fixed order
          res[tt] = tot;
        }
      }
      __syncthreads();
    }
    if (GW > 1 && first) {  // placement check (see k_cg_onchip4): plain-store hand-off only when the group shares an XCD
      unsigned xc = xcc;
      asm volatile("" : "+s"(xc));
      same_xcd = same_xcd_verdict(res[2 * RC + 4], res[2 * RC + 5], GW, xc, a.allow_l2_handoff);
    }
    first = false;
    if (stamp) a.dbg[2] = wall_clock64();
    const int64_t b_next = (int64_t)res[2 * RC + 2];
    {
      int tp = t;
      asm volatile("" : "+v"(tp));
      if (b_next < a.B) {
        request(flip ? a.B - 1 - b_next : b_next, tp, 0, std::integral_constant<int, NPF>{}, pre);
      } else {  // (defined on both paths: no value of the finished members stays live)
#pragma unroll
        for (int i = 0; i < NPF; ++i) pre[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    if (a.prefetch & 1) __builtin_amdgcn_s_setprio(3);

    // ---- the iterations: the chain of k_cg_rspace<.., true> (lo_rspace.hip), operation for operation ----
    const int j = lane & 31, hf = lane >> 5;
    const bool live = j < RC;
    const int jr = live ? j : RC - 1;
    double yj = 0.0, xi = 0.0;
    float nrm;
    {
      double a0 = res[2 * RC + 1], s = res[2 * RC];
      const double d2 = res[2 * RC + 3];
      nrm = sqrtf((float)a0);                             // rhs.norm(2, dim=-2)          :177
      const bool rhs_zero = nrm < a.eps;                  // :178
      if (rhs_zero) nrm = 1.0f;                           // :179
      const double inv = 1.0 / (double)nrm;
      const double w0 = live ? res[jr] * inv : 0.0, u0 = live ? res[RC + jr] * inv : 0.0;
      s *= inv * inv;
      a0 *= inv * inv;
      // r^T r >= r.z / max(dinv) >= r.z / sqrt(sum dinv^2): above this r.z the has_converged mask (:300, 1e-10) cannot hold
      float sa = a.stop_after;
      asm volatile("" : "+s"(sa));
      const double sure_rz = 2.0 * (double)sa * (double)sa * sqrt(d2);
      double* myv = gv[wave];
      if (hf == 0) myv[j] = w0;
      __builtin_amdgcn_wave_barrier();
      const double* row0m = mat_s + (size_t)jr * MLD + hf * NH;                    // row j of TinT (this half)
      // c0 = TinT w0 = W^T beta0, g0 = TuT w0 = W^-1 beta0 (beta0 = U^T b^): |beta0|^2 = c0 . g0 and V S^-1 beta0 = Tin g0
      double c0 = own_row_dot<NH>(row0m, myv + hf * NH);                           // TinT w0
      double e0 = own_row_dot<NH>(row0m + (size_t)1 * RC * MLD, myv + hf * NH);    // g0 = TuT w0
      const double* nrow = row0m + (size_t)2 * RC * MLD;                           // row j of G2 = C^T C
      const double* tucol = mat_s + (size_t)(1 * RC + hf * NH) * MLD + jr;         // column j of TuT (this half of its rows)
      c0 = live ? c0 : 0.0;
      e0 = live ? e0 : 0.0;
      double tau2 = s - lanes32_sum_d(c0 * e0);            // |b_perp|^2 = s - |beta0|^2
      tau2 = tau2 > 0.0 ? tau2 : 0.0;
      // a right-hand side (almost) inside span(C) asks for the dense form (CgCtrl::rs_redo; lo_rspace.hip)
      const bool delicate = !rhs_zero && tau2 < 1e-2 * s;
      const double lam = live ? lam_mine : 1.0;
      long long ts_a = 0, ts_b = 0;
      if (stamp) ts_a = wall_clock64();
      double cj = c0, qj = 0.0, etaj = 0.0;
      double cp = 1.0, qp = 0.0, etap = 0.0;
      double rz = 0.0, pApE = 0.0, alpha = 0.0, beta = 0.0;
      float rn = 0.f, last_alpha = 0.f;
      bool conv = false;
      unsigned close_flags = 0u;
      const size_t bc = (size_t)m;
      const bool rec = wig == 0 && lane == 0;
      const int last_owner = (a.iters - 1) & 3;  // the wave that forms the last residual norm writes the member's state
      // The last iteration's residual norm enters nothing but the member's records (resid_rec, resid_norm, has_conv, the
      // close granule): x took its last update at the top of that iteration, the alpha its `conv` would zero is never
      // applied.  It is 150 instructions with eight serialized LDS round trips on the path to y, so
      //   * only workgroup 0 of a group, which stores the records, forms it at all;
      //   * for a member that is not the group's final one, the owning wave leaves del and c' in late_v and forms the
      //     norm at the next member's top, behind that member's requests, where all waves wait for loads (the group's
      //     final member keeps the order norm, records, closing step, x pass: the closing step reads the granule).
      const bool late = wig == 0 && a.iters > 0 && wave_u == last_owner &&
                        __builtin_amdgcn_readfirstlane((int)(b_next < a.B)) != 0;  // (wave-uniform)
      for (int kk = -1; kk < a.iters; ++kk) {
        if (kk >= 0) {  // x += alpha p (:31);  r -= alpha A p (:264)
          last_alpha = (float)alpha;
          etaj = fma(alpha, qj, etaj);
          etap = fma(alpha, qp, etap);
          cj = fma(-alpha * lam, qj, cj);
          cp = fma(-alpha, qp, cp);
        }
        const double lc = lam * cj;
        // three sums over the components in one pass: the lower half-wave carries c.c and c.lam c, the upper c.lam q
        const bool lo_h = hf == 0;
        const float inv_rz = __builtin_amdgcn_rcpf((float)rz);       // (off the chain: rz is the previous iteration's)
        const double red2 = row16_sum_d(halve_pair_d<16>(lo_h ? cj * cj : lc * qj, lo_h ? lc * cj : 0.0, lane));
        const double cc = pick_d(red2, 0), clc = pick_d(red2, 16), clq = pick_d(red2, 32);
        const double rzn = fma(cp * cp, tau2, cc);                     // residual_inner_prod :215 / :35-36
        const bool sure = rzn > sure_rz;
        const bool rec_first = kk == 0 && a.close_gran == nullptr && wave == 0;
        const bool rec_last = kk == a.iters - 1 && wave == last_owner && wig == 0;
        const bool late_now = late && kk == a.iters - 1;               // (this wave's rec_last, formed at the next member's top)
        const bool own = rec_first || rec_last || !sure;
        float rnn = 0.f;
        if (kk < 0) {
          const float s1f = (float)a0;
          rnn = __builtin_amdgcn_sqrtf(s1f < 0.f ? 0.f : s1f);
        } else if (late_now) {
          const double dl = fma(-cp, c0, cj);                          // del = c - c' c0
          if (hf == 0) late_v[j] = dl;
          if (lane == 0) late_v[32] = cp;
        } else if (own) {
          const double dl = fma(-cp, c0, cj);                          // del = c - c' c0
          rnn = resid_norm_c<NH, MLD>(dl, cp, a0, u0, live, j, hf, lane, myv, tucol, nrow);
        }
        if (kk >= 0) {                                               // closes iteration kk: beta, residual norm, records
          beta = ((float)rz < a.eps) ? 0.0 : (double)((float)rzn * inv_rz);  // :39-42
          if (rhs_zero) rnn = 0.f;                                   // :299
          rn = rnn;
          if (rec && (rec_first || rec_last) && !late_now) {
            long long nb = a.B;  // (opaque: the record's offset is formed here, not kept -- and spilled -- around the loops)
            asm volatile("" : "+s"(nb));
            a.resid_rec[(size_t)kk * (size_t)nb + bc] = rn;
          }
        } else {
          beta = 0.0;
          rn = rnn;
          if (wig == 0 && t == 0) a.init_conv[bc] = (rn < a.stop_after) ? 1 : 0;  // :204-205
          close_flags = ((rn < a.stop_after) ? 1u : 0u) | (delicate ? 4u : 0u);
          if (delicate && rec && wave == 0) atomicOr(a.err + 4, 1);  // (CgCtrl::rs_redo, for the host-launched control step)
        }
        // (NaN after the first product, linear_cg.py:199-200: the residual norm is NaN exactly when the coordinates are)
        if (kk == 0 && (rnn != rnn || rzn != rzn)) close_flags |= 2u;
        conv = (own || rhs_zero) ? (rn < a.stop_after) : false;      // :300
        rz = rzn;
        // p = z + beta p (:268, :46);  p.Ap = sum lam (c + beta q)^2 + q'^2 tau2
        pApE = fma(beta, fma(beta, pApE, 2.0 * clq), clc);
        qj = fma(beta, qj, cj);
        qp = fma(beta, qp, cp);
        const double pAp = fma(qp * qp, tau2, pApE);
        alpha = ((float)pAp < a.eps) ? 0.0 : (double)((float)rz * __builtin_amdgcn_rcpf((float)pAp));  // :254-257
        if (conv) alpha = 0.0;                                       // :260
      }
      if (stamp) ts_b = wall_clock64();
      if (rec && wave == last_owner) {
        a.rhs_norm[bc] = nrm;
        a.rhs_is_zero[bc] = rhs_zero ? 1 : 0;
        a.rz[bc] = (float)rz;
        a.alpha[bc] = last_alpha;
        a.beta[bc] = (float)beta;
        if (late) {  // (residual norm, has_conv and the close granule: at the next member's top)
          late_v[33] = (double)close_flags;
          late_v[34] = (double)m;
        } else {
          a.resid_norm[bc] = rn;
          a.has_conv[bc] = conv ? 1 : 0;
          if (a.close_gran) {
            granule_store(a.close_gran + m, granule_pack(a.close_epoch | close_flags, rn), /*same_xcd=*/false);
          }
        }
      }
      // y = Tin (eta - xi g0): lane i walks column i of TinT (its half of the eigen-indices)
      __builtin_amdgcn_wave_barrier();
      if (hf == 0) myv[j] = fma(-etap, e0, etaj);
      __builtin_amdgcn_wave_barrier();
      xi = etap;
      {
        const double* col = mat_s + (size_t)(hf * NH) * MLD + jr;
        // (every LDS read of the walk in flight before the first FMA: the chain's state is dead, its registers hold them.
        //  Read as they were needed, each ds_read2_b64 had its own s_waitcnt: NH / 2 LDS round trips in a row)
        double cv[NH];
        double2 ee[NH / 2];
#pragma unroll
        for (int q = 0; q < NH; q += 2) {
          ee[q / 2] = *reinterpret_cast<const double2*>(myv + hf * NH + q);
          cv[q] = col[(size_t)q * MLD];
          cv[q + 1] = col[(size_t)(q + 1) * MLD];
        }
        __builtin_amdgcn_sched_barrier(0);
        double a0_ = 0.0, a1_ = 0.0;
#pragma unroll
        for (int q = 0; q < NH; q += 2) {  // (the same FMAs in the same order)
          a0_ = fma(cv[q], ee[q / 2].x, a0_);
          a1_ = fma(cv[q + 1], ee[q / 2].y, a1_);
        }
        double lo_, up_;
        halves_d(a0_ + a1_, lo_, up_);
        yj = lo_ + up_;
      }
      yj = live ? yj : 0.0;
      if (stamp) {  // (printed as wg-wait / publish / poll: start of the chain, the iterations, y)
        a.dbg[5] = ts_a - a.dbg[2];
        a.dbg[6] = ts_b - ts_a;
        a.dbg[7] = wall_clock64() - ts_b;
      }
      // every wave writes nrm * y for its own x pass
      __builtin_amdgcn_wave_barrier();
      if (hf == 0) myv[j] = yj * (double)nrm;
      __builtin_amdgcn_wave_barrier();
    }
    // ---- the group's final member: close the solve HERE, in front of the x pass (lo_cg_close.h) ----
    // The closing step reads the members' close granules, the error word and the counters, nothing of x: the host's
    // ticket need not wait for this pass (2.3 - 2.5 us), and x was complete in stream order only before as well (the
    // ticket used to leave after workgroup 0's own x pass, with the group's other workgroups still storing).  Why the
    // helper's conditions hold at this point:
    //   (1) b_next = ngroups + the value this member's draw returned, and it is >= B: the group's LAST draw from
    //       next_member has returned (the loop ends with this member, nobody of the group draws again);
    //   (2) the exchange above was the group's last, and workgroup 0 saw the granules of all GW workgroups in it: a
    //       sibling that is still polling them can only find them, so nobody of this group sets the error word any more;
    //   (3) the member's state and close granule were stored behind the chain above (a final member never defers them).
    //       Those of the group's earlier members were issued at the top of the member that followed each, in front of
    //       that member's barrier: every wave of this workgroup has passed those barriers.  (The call sits behind y, not behind
    //       the stores: here only C, xi and the stage pointers are live.)
    // Uniform over the workgroup (res[] is LDS, wig and po.n are scalars): the barriers inside the helper are legal.
    // With peer buffers the close stays behind the x pass: a rank that has seen its solve return has issued its peer stores.
    if (a.close_gran && wig == 0 && po.n == 0 && __builtin_amdgcn_readfirstlane((int)(b_next >= a.B))) {
      int tc = (int)threadIdx.x;  // (opaque: what the helper derives from it is formed here, not kept around the loop)
      asm volatile("" : "+v"(tc));
      cg_close_solve(a, ngroups, tc);
      closed = 1;
      // (no next member: pre[] holds zeros.  Defined again behind the call, its 32 registers are dead across it and
      //  the closing step needs none that C or the x pass occupy: 0 spills)
#pragma unroll
      for (int i = 0; i < NPF; ++i) pre[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (!(a.prefetch & 2)) __builtin_amdgcn_s_setprio(0);
    if (stamp) a.dbg[3] = wall_clock64();
    // ---- x = nrm D^-1 (xi r0 + C y) = D^-1 (xi b + C (nrm y)), fp64 (for small diagonals the two terms cancel) ----
    {
      int l2 = lane;
      asm volatile("" : "+v"(l2));
      const int k2 = l2 & (CH - 1), g2 = l2 / CH;
      const double* myv = gv[wave];
      const double2 ya = *reinterpret_cast<const double2*>(&myv[4 * k2]);
      const double2 yb = *reinterpret_cast<const double2*>(&myv[4 * k2 + 2]);
      g_f* const xb = opaque_uniform((g_f*)(a.xout + (size_t)m * a.N + row0c));
      const bool more = b_next < a.B;
      const int64_t m_next = flip ? a.B - 1 - b_next : b_next;
      g_cc* const Cn = (g_cc*)(a.C + ((size_t)(more ? m_next : m) * a.N + row0c) * RC);
      const unsigned loffn = (unsigned)((g2 * RC + 4 * k2) * sizeof(float));
#pragma unroll
      for (int js = 0; js < 4; ++js) {
        constexpr int J0 = NPF / CH;        // first group behind the prefetched instructions
        const int jj = (js + J0) & 3;       // (compile-time after unrolling)
        double p[CH];
#pragma unroll
        for (int m = 0; m < CH; ++m) {
          const f32x4 c4 = Cr[CH * jj + m];
          p[m] = fma((double)c4.w, yb.y, fma((double)c4.z, yb.x, fma((double)c4.y, ya.y, (double)c4.x * ya.x)));
        }
        const double xv = rows_reduce_d<CH>(p, l2);
        const int rw = 64 * jj + RPI * k2 + g2;
        const int row = row0c + rw;
        const double acc = fma(xi, (double)bw[rw], xv);
        if (row >= row0 && row < a.N) {
          const float xval = (float)(acc * (double)dw[rw]);  // :335
          xb[rw] = xval;
          for (int pp = 0; pp < po.n; ++pp)  // (prototype: the gather as peer writes)
            ((g_f*)po.buf[pp])[((size_t)(m + po.member_off)) * a.N + row] = xval;
        }
        if (CH * jj >= NPF) {  // the registers of this group are free: the next member's rows of the same instructions
          g_cc* bqn = opaque_uniform(Cn + (CH * jj + 4) * 1024);
#pragma unroll
          for (int m = 0; m < CH; ++m)
            nxt[CH * jj - NPF + m] = more ? *(g_cf4*)(bqn + loffn + (m - 4) * 1024) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_s_setprio(0);
    if (stamp) a.dbg[4] = wall_clock64();
    // (no barrier here: the one that releases mat_s and res[] to the next member stands behind its requests, above)
    late_pending = wig == 0 && a.iters > 0 && __builtin_amdgcn_readfirstlane((int)(b_next < a.B)) != 0;
    b = b_next;
  }
  // (not closed yet: a group that never entered the loop -- fewer members than groups --, or peer buffers installed)
  if (a.close_gran && wig == 0 && !closed) {
    int te = (int)threadIdx.x;
    asm volatile("" : "+v"(te));
    cg_close_solve(a, ngroups, te);
  }
}

// LO_RS_PRIO: wave-priority mask of the latency-critical phases, read once per process
int rspace3_prio() {
  static const int prio = [] {
    const char* e = getenv("LO_RS_PRIO");
    return e ? atoi(e) : 3;  // iterations AND the x pass at raised priority (0.1935 -> 0.1894 ms per headline solve)
  }();
  return prio;
}

// ---- the hand-off block the library owns (one per device) ----
// What a launch of k_cg_rspace3 shares between its workgroups -- the error word, the member hand-out counter, the close
// counter, the exchange granules and the close granules -- used to be carved out of the caller's workspace, which may be
// fresh memory on every call: one k_zero_span launch in front of every solve (2.3 us + a 4 us dependent-launch gap in front
// of a 142 us kernel, profiles/r07).  Here they live in a buffer that is allocated and zeroed ONCE (as k_lr_mv's,
// lo_lowrank_mv.hip) and told apart launch from launch:
//   * exchange granules carry tags above `tag_base`, which grows by more than a workgroup can perform exchanges in a launch
//     (one per member it takes: at most B);
//   * close granules carry the launch's epoch in the bits above the member's three flags;
//   * the two counters are left at zero by the closing workgroup (lo_cg_close.h), the error word stays zero while nothing
//     is lost.
// The block is cleared again (the old way: zero_span in front of the launch) when a counter would wrap, and when the
// previous launch on it was not CONFIRMED clean by the host (handoff_launch_confirm): a lost hand-off, an injected one, a
// launch error, a caller that gave up on the ticket.  Resident launches of a process never overlap (ResidentLaunch),
// whose lock also guards this state.
constexpr size_t HO_MAX_WGS = 2 * 320;           // two workgroups per CU, up to 320 CUs
constexpr size_t HO_GRAN_PER_WG = 432;           // (rspace_gbuf_bytes: what a workgroup's share of a group's granules may take)
constexpr size_t HO_MAX_MEMBERS = 65536;         // close granules; larger batches take the caller's workspace
constexpr size_t HO_HEAD_BYTES = 256;            // err | next_member | close_count | . | (err + 4: rs_redo of the host-closed form, unused)
constexpr unsigned HO_TAG_LIMIT = 0xfff00000u;   // tag_base + B + 2 stays below it
constexpr unsigned HO_EPOCH_LIMIT = 0x1ffffff0u; // epochs are 29-bit and never 0
struct HandoffBlock {
  char* buf = nullptr;
  size_t bytes = 0;
  bool failed = false;
  unsigned next_tag = 1, next_epoch = 1;
  unsigned last_launch = 0;                 // id of the last launch on the block (0: none yet)
  std::atomic<unsigned> confirmed{0};       // id of the last launch the host saw closing clean
  bool force_clear = false;                 // lo_resident_handoff_debug: the next launch clears the block
  unsigned clears = 0, launches = 0;        // (lo_resident_handoff_debug)
  // The walk order of the members (OnchipArgs::member_flip).  A solve streams its whole operator, 1.05 MB a member at
  // the headline shape, and the memory-side cache (256 MiB, allocates on streamed reads) keeps roughly the bytes read
  // last.  Walked the same way every time, a solve starts with the members the previous one read longest ago: all
  // evicted.  So an owned launch on the operator of the last owned launch -- same C, B, N and RC -- runs in the opposite
  // direction when that launch was confirmed clean, and every other launch runs forward.  The order never enters a
  // result: a record that is stale or matches by accident costs nothing but the hits.
  const float* ord_C = nullptr;             // operator of the last owned launch (null: none)
  int64_t ord_B = 0;
  int ord_N = 0, ord_RC = 0;
  bool ord_flip = false;                    // its direction
  int ord_mode = 0;                         // lo_resident_order_debug: 0 automatic, 1 always forward, 2 always reverse
  unsigned ord_last = 0, ord_reversed = 0;  // direction of the last k_cg_rspace3 launch (owned or not), reversed launches
  // The ordered start (OnchipArgs::start_delay, lo_rs3_start.h): lo_resident_start_debug sets mode and delta, every launch
  // of k_cg_rspace3 -- owned or not -- records the argument it ran with and the groups it was laid out in.
  int start_mode = R3_START_AUTO, start_delta = 0;
  int start_last = 0, start_last_ngroups = 0;
  unsigned start_waited = 0;                // launches that ran with a wait
};
HandoffBlock g_handoff[16];
std::atomic<unsigned> g_handoff_ids{0};

HandoffBlock* handoff_block() {  // (called with the ResidentLaunch lock held)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  HandoffBlock& h = g_handoff[dev];
  if (!h.buf && !h.failed) {
    h.bytes = HO_HEAD_BYTES + (HO_MAX_WGS * HO_GRAN_PER_WG + HO_MAX_MEMBERS) * sizeof(unsigned long long);
    if (hipMalloc(&h.buf, h.bytes) != hipSuccess || hipMemset(h.buf, 0, h.bytes) != hipSuccess) {
      (void)hipGetLastError();
      h.buf = nullptr;
      h.failed = true;
    }
  }
  return h.buf ? &h : nullptr;
}

// The counters of the next launch on the block: true when the block has to be cleared first (wrap-around).
bool handoff_advance(unsigned* next_tag, unsigned* next_epoch, int64_t B, unsigned* tag_base, unsigned* epoch) {
  bool wrap = false;
  const unsigned need = (unsigned)B + 2u;  // (B <= HO_MAX_MEMBERS)
  if (*next_tag >= HO_TAG_LIMIT - need || *next_epoch >= HO_EPOCH_LIMIT) {
    *next_tag = 1;
    *next_epoch = 1;
    wrap = true;
  }
  *tag_base = *next_tag;
  *epoch = *next_epoch;
  *next_tag += need;
  *next_epoch += 1;
  return wrap;
}

struct OwnedLaunch {  // rspace3_go: null for a launch on the caller's (cleared) workspace
  bool inject;
  unsigned* launch_id;
};

template <int RC, int GW>
int rspace3_go(const OnchipArgs& a, int nwg, const OwnedLaunch* own, hipStream_t st) {
  int per_cu = 0;
  if (LO_OCCUPANCY_CACHED(per_cu, (k_cg_rspace3<RC, GW>), R3_TPB, 0) != hipSuccess || per_cu < 2) return LO_ERR_UNSUPPORTED;
  LO_PROF_BEGIN("cg_onchip", st);  // (one scope for the resident single-column kernels: lo_cg_last_executed tells them apart)
  ResidentLaunch guard(st);
  OnchipArgs a2 = a;
  a2.prefetch = rspace3_prio();
  a2.member_flip = 0;
  int dev = 0;  // (the order state of a launch on the caller's workspace: the device's block record, without its buffer)
  HandoffBlock* const ho = (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16) ? &g_handoff[dev] : nullptr;
  if (own) {
    // (host-assigned tags must not be baked into a captured graph: a replay would meet its own granules)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      return LO_ERR_UNSUPPORTED;
    }
    HandoffBlock* h = (a.B <= (int64_t)HO_MAX_MEMBERS && (size_t)2 * nwg <= HO_MAX_WGS) ? handoff_block() : nullptr;
    if (!h) return LO_ERR_UNSUPPORTED;
    const bool prev_clean = h->last_launch != 0 && h->last_launch == h->confirmed.load(std::memory_order_acquire);
    bool clear = h->force_clear || h->last_launch != h->confirmed.load(std::memory_order_acquire);
    h->force_clear = false;
    // (see HandoffBlock: the opposite direction on the operator of a clean predecessor, forward otherwise)
    const bool same_op = h->ord_C == a.C && h->ord_B == a.B && h->ord_N == a.N && h->ord_RC == RC;
    a2.member_flip = (same_op && prev_clean && !h->ord_flip) ? 1 : 0;
    h->ord_C = a.C; h->ord_B = a.B; h->ord_N = a.N; h->ord_RC = RC;
    clear = handoff_advance(&h->next_tag, &h->next_epoch, a.B, &a2.tag_base, &a2.close_epoch) || clear;
    h->last_launch = g_handoff_ids.fetch_add(1, std::memory_order_relaxed) + 1;
    if (h->last_launch == 0) h->last_launch = g_handoff_ids.fetch_add(1, std::memory_order_relaxed) + 1;
    *own->launch_id = h->last_launch;
    ++h->launches;
    if (clear) {  // (ordered behind every earlier resident launch by the guard)
      ++h->clears;
      const int zrc = zero_span(h->buf, h->bytes, st);
      if (zrc) return zrc;
    }
    a2.close_epoch <<= 3;
    a2.handoff_owned = 1;
    a2.err = reinterpret_cast<int*>(h->buf);
    a2.next_member = a2.err + 1;
    a2.close_count = a2.err + 2;
    a2.gbuf = reinterpret_cast<unsigned long long*>(h->buf + HO_HEAD_BYTES);
    a2.close_gran = a2.gbuf + HO_MAX_WGS * HO_GRAN_PER_WG;
    if (own->inject) LO_HIP_CHECK(hipMemsetAsync(a2.err, 1, 1, st));
  }
  if (ho) {
    if (ho->ord_mode) a2.member_flip = ho->ord_mode == 2 ? 1 : 0;  // (forced: owned and other launches alike)
    if (own) ho->ord_flip = a2.member_flip != 0;
    ho->ord_last = (unsigned)a2.member_flip;
    ho->ord_reversed += (unsigned)a2.member_flip;
  }
  // (the ordered start: by the rounds of this launch, or as lo_resident_start_debug forces it)
  const int ngroups = (2 * nwg / 8 / GW) * 8;
  a2.start_delay = r3_start_arg(ho ? ho->start_mode : R3_START_AUTO, ho ? ho->start_delta : 0, a.B, ngroups);
  if (ho) {
    ho->start_last = a2.start_delay;
    ho->start_last_ngroups = ngroups;
    ho->start_waited += a2.start_delay != 0 ? 1u : 0u;
  }
  PeerOut po;
  {
    std::lock_guard<std::mutex> lk(g_peer_mu);
    po = g_peer_out;
  }
  hipLaunchKernelGGL((k_cg_rspace3<RC, GW>), dim3(2 * nwg), dim3(R3_TPB), 0, st, a2, po);
  LO_PROF_END(st);
  LO_LAUNCH_CHECK();
  return LO_OK;
}

template <int RC>
int rspace3_gw(const OnchipArgs& a, int nwg, const OwnedLaunch* own, hipStream_t st) {
  switch (a.GW) {
    case 1: return rspace3_go<RC, 1>(a, nwg, own, st);
    case 2: return rspace3_go<RC, 2>(a, nwg, own, st);
    case 4: return rspace3_go<RC, 4>(a, nwg, own, st);
    case 8: return rspace3_go<RC, 8>(a, nwg, own, st);
    case 16: return rspace3_go<RC, 16>(a, nwg, own, st);
    case 32: return rspace3_go<RC, 32>(a, nwg, own, st);
  }
  return LO_ERR_UNSUPPORTED;
}

int rspace3_dispatch(int RC, const OnchipArgs& a, int nwg, const OwnedLaunch* own, hipStream_t st) {
  if (!a.RSD || a.x || a.c != 1 || a.ab_rec || !a.xout || a.GW > 32 || a.N < 256 || (int64_t)a.GW * R3_ROWS < a.N)
    return LO_ERR_UNSUPPORTED;
  // granules of a group: 2 x GW x NP x 2 -- inside what rspace_gbuf_bytes reserves per workgroup (432)
  if (RC == 32) return rspace3_gw<32>(a, nwg, own, st);
  if (RC == 16) return rspace3_gw<16>(a, nwg, own, st);
  if (RC == 8) return rspace3_gw<8>(a, nwg, own, st);
  return LO_ERR_UNSUPPORTED;
}

}  // namespace

// The diagonal form in the chunk-per-lane layout: groups of up to 32 workgroups (N <= 32768), members of at least 256 rows,
// rows per workgroup = 1024 (a.RW).  LO_ERR_UNSUPPORTED: rspace_launch runs k_cg_rspace<.., true>.
int rspace3_launch(int RC, const OnchipArgs& a, int nwg, hipStream_t st) { return rspace3_dispatch(RC, a, nwg, nullptr, st); }

int rspace3_launch_owned(int RC, const OnchipArgs& a, int nwg, bool inject, unsigned* launch_id, hipStream_t st) {
  if (!a.close_gran || !a.close_ctrl || !a.close_mirror || a.dbg) return LO_ERR_UNSUPPORTED;
  const OwnedLaunch own = {inject, launch_id};
  return rspace3_dispatch(RC, a, nwg, &own, st);
}

void handoff_launch_confirm(unsigned launch_id) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return;
  g_handoff[dev].confirmed.store(launch_id, std::memory_order_release);
}

}  // namespace lo

extern "C" int lo_peer_gather_set(float* const* bufs, int n, long long member_offset) {
  if (n < 0 || n > 7 || (n > 0 && !bufs)) return LO_ERR_BADARG;
  std::lock_guard<std::mutex> lk(lo::g_peer_mu);
  for (int i = 0; i < 7; ++i) lo::g_peer_out.buf[i] = i < n ? bufs[i] : nullptr;
  lo::g_peer_out.n = n;
  lo::g_peer_out.member_off = member_offset;
  return LO_OK;
}

// Test / debug access to the hand-off block of the current device (lo_amd.h).
extern "C" int lo_resident_handoff_debug(int32_t force_clear, int64_t set_next_tag, int64_t set_next_epoch, uint32_t* out) {
  lo::ResidentLock guard;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return LO_ERR_BADARG;
  lo::HandoffBlock& h = lo::g_handoff[dev];
  if (set_next_tag > 0xffffffffll || set_next_epoch > 0xffffffffll) return LO_ERR_BADARG;
  if (set_next_tag >= 0) h.next_tag = (unsigned)set_next_tag;
  if (set_next_epoch >= 0) h.next_epoch = (unsigned)set_next_epoch;
  if (force_clear) h.force_clear = true;
  if (out) {
    out[0] = h.next_tag;
    out[1] = h.next_epoch;
    out[2] = h.clears;
    out[3] = h.launches;
  }
  return LO_OK;
}

// Test / debug access to the walk order of k_cg_rspace3 on the current device (lo_amd.h).
extern "C" int lo_resident_order_debug(int32_t mode, uint32_t* out) {
  lo::ResidentLock guard;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return LO_ERR_BADARG;
  if (mode < -1 || mode > 2) return LO_ERR_BADARG;
  lo::HandoffBlock& h = lo::g_handoff[dev];
  if (mode >= 0) h.ord_mode = mode;
  if (out) {
    out[0] = h.ord_last;
    out[1] = h.ord_reversed;
  }
  return LO_OK;
}

// Test / debug access to the ordered start of k_cg_rspace3 on the current device (lo_amd.h).
extern "C" int lo_resident_start_debug(int32_t mode, int32_t delta_ticks, uint32_t* out) {
  lo::ResidentLock guard;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return LO_ERR_BADARG;
  if (mode < -1 || mode > lo::R3_START_GIVEN) return LO_ERR_BADARG;
  const bool given = mode == lo::R3_START_GIVEN;
  if (given && (delta_ticks < 0 || delta_ticks > lo::R3_START_CAP_TICKS)) return LO_ERR_BADARG;
  lo::HandoffBlock& h = lo::g_handoff[dev];
  if (mode >= 0) {
    h.start_mode = mode;
    h.start_delta = given ? delta_ticks : 0;
  }
  if (out) {
    out[0] = (uint32_t)h.start_mode;
    out[1] = (uint32_t)h.start_last;
    out[2] = (uint32_t)h.start_last_ngroups;
    out[3] = h.start_waited;
  }
  return LO_OK;
}

// The rule of the ordered start without a device: the ticks group `grp` of a launch of B members in `ngroups` groups waits.
extern "C" int lo_resident_start_delay(int32_t mode, int32_t delta_ticks, int64_t B, int32_t ngroups, int32_t grp) {
  if (mode < 0 || mode > lo::R3_START_GIVEN || B < 0 || ngroups < 8 || ngroups % 8 || grp < 0 || grp >= ngroups) return -1;
  return lo::r3_start_delay(lo::r3_start_arg(mode, delta_ticks, B, ngroups), grp, ngroups / 8);
}
