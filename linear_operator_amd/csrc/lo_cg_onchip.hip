// lo_cg_onchip.hip -- what the operator-resident kernels share on the host side: the ordering of resident launches across
// streams (ResidentLaunch), the workgroup count they are sized by (onchip_num_workgroups, LO_OC_RESERVE_CUS), the opt-in of
// the same-XCD plain-store hand-off, the granule budget of the serial kernels.
// (Rounds 1 - 5 also kept the FIRST generation of the resident CG here -- k_cg_onchip: one row per thread, C in LDS, four
// group all-reduces per iteration, 0.95 ms per headline solve.  Nothing had selected it since k_cg_onchip4 (round 1) and
// k_cg_onchip5 (round 2); removed in round 6 with its plan rows.  The design notes of the hand-off -- tagged 8-byte
// granules, two slot sets by phase parity, bounded polls -- live in lo_group_reduce.h and DESIGN.md 4.2.)
#include <algorithm>
#include <mutex>
#include <stdlib.h>
#include <unistd.h>  // environ

#include "lo_device.h"
#include <string.h>

#include "lo_internal.h"
#include "lo_cg_onchip.h"

namespace lo {

constexpr int OC_GW = 8;  // (granule budget of the serial resident kernels: groups of up to 8 x 40 granules per parity)

size_t onchip_gbuf_bytes(int ngroups) { return (size_t)ngroups * 2 * OC_GW * 40 * sizeof(unsigned long long); }

namespace {
std::mutex g_res_mu;
hipStream_t g_res_last = nullptr;
int g_res_last_dev = -1;
bool g_res_have = false;
hipEvent_t g_res_ev[16] = {};
}  // namespace

// ---- the LO_* switches (lo_internal.h) ----
static CgEnv env_pass() {
  enum { kNoLockstep, kGw8, kKeepState, kNoRspaceCols, kNoRspace, kNoWrec, kNoKronRoot, kNoFusedCtrl, kTestFallback,
         kRsNoDiag, kClearHandoff, kScTestFallback, kLsDebug, kOcDebug, kScDebug, kNoL2Handoff, kReserveCus,
         kNoResidentOrder, kCount };
  static const char* const names[kCount] = {
      "OC_NO_LOCKSTEP", "OC_GW8", "OC_KEEP_STATE", "NO_RSPACE_COLS", "OC_NO_RSPACE", "OC_NO_WREC", "NO_KRON_ROOT",
      "NO_FUSED_CTRL", "OC_TEST_FALLBACK", "RS_NO_DIAG", "OC_CLEAR_HANDOFF", "SC_TEST_FALLBACK", "LS_DEBUG", "OC_DEBUG",
      "SC_DEBUG", "OC_NO_L2_HANDOFF", "OC_RESERVE_CUS", "NO_RESIDENT_ORDER"};
  const char* val[kCount] = {};
  for (char** e = environ; e && *e; ++e) {
    const char* v = *e;
    if (v[0] != 'L' || v[1] != 'O' || v[2] != '_') continue;
    const char* eq = strchr(v + 3, '=');
    if (!eq) continue;
    const size_t len = (size_t)(eq - (v + 3));
    for (int i = 0; i < kCount; ++i)
      if (!val[i] && strlen(names[i]) == len && memcmp(names[i], v + 3, len) == 0) {  // (the first match, as getenv)
        val[i] = eq + 1;
        break;
      }
  }
  CgEnv env;
  auto on = [&](int i) { return val[i] != nullptr; };
  env.sw.no_lockstep = on(kNoLockstep); env.sw.gw8 = on(kGw8); env.sw.keep_state = on(kKeepState);
  env.sw.no_rspace_cols = on(kNoRspaceCols); env.sw.no_rspace = on(kNoRspace); env.sw.no_wrec = on(kNoWrec);
  env.sw.no_kron_root = on(kNoKronRoot); env.sw.no_fused_ctrl = on(kNoFusedCtrl);
  env.sw.oc_test_fallback = on(kTestFallback); env.sw.rs_no_diag = on(kRsNoDiag); env.sw.clear_handoff = on(kClearHandoff);
  env.sw.sc_test_fallback = val[kScTestFallback] ? atoi(val[kScTestFallback]) : -1;
  env.ls_debug = on(kLsDebug); env.oc_debug = on(kOcDebug); env.sc_debug = on(kScDebug);
  env.ls_member = env.ls_debug ? atoi(val[kLsDebug]) : 0;
  env.oc_member = env.oc_debug ? atoi(val[kOcDebug]) : 0;
  env.no_l2_handoff = on(kNoL2Handoff);
  env.has_reserve = on(kReserveCus);
  env.reserve_cus = env.has_reserve ? atoi(val[kReserveCus]) : 0;
  env.no_resident_order = on(kNoResidentOrder);
  return env;
}
static thread_local CgEnv tls_env;
static thread_local int tls_env_depth = 0;
CgEnv cg_env() { return tls_env_depth > 0 ? tls_env : env_pass(); }
EnvScope::EnvScope() {
  if (tls_env_depth++ == 0) tls_env = env_pass();
}
EnvScope::~EnvScope() { --tls_env_depth; }

ResidentLaunch::ResidentLaunch(hipStream_t st) {
  g_res_mu.lock();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return;
  if (g_res_have && g_res_last_dev == dev && g_res_last != st && !cg_env().no_resident_order) {
    if (!g_res_ev[dev] && hipEventCreateWithFlags(&g_res_ev[dev], hipEventDisableTiming) != hipSuccess) g_res_ev[dev] = nullptr;
    // (a stream the caller has destroyed in the meantime makes the record fail: nothing left to wait for)
    if (g_res_ev[dev] && hipEventRecord(g_res_ev[dev], g_res_last) == hipSuccess)
      (void)hipStreamWaitEvent(st, g_res_ev[dev], 0);
    else
      (void)hipGetLastError();
  }
  g_res_last = st;
  g_res_last_dev = dev;
  g_res_have = true;
}

ResidentLaunch::~ResidentLaunch() { g_res_mu.unlock(); }

ResidentLock::ResidentLock() { g_res_mu.lock(); }
ResidentLock::~ResidentLock() { g_res_mu.unlock(); }

// The same-XCD hand-off publishes granules with WORKGROUP-scope stores that other workgroups of the XCD read through the
// shared L2: outside the HIP memory model, correct only where a CU's vector L1 is write-through into the XCD's L2.  That
// holds on gfx950 (verified on MI355X: tools/fuzz_resident.py, the GPU test suite) -- so the path is OPT-IN per
// verified architecture string; anywhere else (and with LO_OC_NO_L2_HANDOFF) every granule is an agent-scope store.
// Cost of the agent-scope stores on MI355X: profiles/r04/l2_handoff_cost.txt.
int onchip_l2_handoff_allowed() {
  if (cg_env().no_l2_handoff) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  static int verified[64] = {0};  // 0 unknown, 1 yes, 2 no
  if (verified[dev] == 0) {
    hipDeviceProp_t prop;
    verified[dev] = 2;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) verified[dev] = 1;
  }
  return verified[dev] == 1 ? 1 : 0;
}

int onchip_num_workgroups() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  // (hipGetDeviceProperties fills a ~1.5 KB structure and costs tens of microseconds: asked once per device)
  static int cu_count[64] = {0};
  if (dev < 0 || dev >= 64) return 0;
  if (cu_count[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cu_count[dev] = n;
  }
  int cus = cu_count[dev];
  // LO_OC_RESERVE_CUS=<n>: leave n CUs' worth of workgroup slots unused so that a concurrently running collective
  // (RCCL's all-gather kernel on its own stream) finds room WITHOUT displacing workgroups of a resident group -- a
  // displaced workgroup stalls its whole group until the other kernel ends.  The spare slots end up scattered over the
  // CUs (the dispatcher balances), each big enough for a 256-thread workgroup of <= 256 VGPRs.
  const CgEnv env = cg_env();
  if (env.has_reserve) cus = std::max(64, cus - std::max(0, env.reserve_cus));
  return (cus / 32) * 32;  // 2 workgroups per CU: a multiple of 8 XCDs x 8 workgroups per group
}

}  // namespace lo
