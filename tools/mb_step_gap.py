"""Where the host's share of the headline step goes (512 x 8192 x 32, one `K.cg_solve` per step):
  (c) Python before the C call   (b) Python after it   (d) entry of the C call -> the launch has returned
  (a) ticket seen -> the C call returns   kernel (HIP events)   (e) the remainder: launch -> kernel start.
(a) and (d) come from the library's own steady_clock pairs (`_hip.prof_enable(2)`, "host:" lines of the report) where the
build has them; (b) and (c) are timed here, piece by piece.  Runs the general path (LO_CG_NO_SESSION=1) and, where the
build has solve sessions, the session path."""
import ctypes as C, os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from linear_operator_amd import _hip, kernels as K
B, N, R = 512, 8192, 32
g = torch.Generator(device="cuda"); g.manual_seed(1)
Cm = torch.randn(B, N, R, generator=g, device="cuda") / R ** 0.5
d = torch.rand(B, N, generator=g, device="cuda") + 0.5
rhs = torch.randn(B, N, 1, generator=g, device="cuda")
desc = K.lowrank_diag_descriptor(Cm, d)
L, perm = K.pivoted_cholesky(desc, 15, contiguous=False)
pre = K.precond_build(L, d, False, root=Cm, perm=perm).ensure_eigform()
lib = _hip.load()
has_sessions = hasattr(lib, "lo_cg_session_solve_f32")
step = lambda: K.cg_solve(desc, rhs, precond=pre, tolerance=1e-4)
def timeit(fn, reps=400):
    for _ in range(20): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter_ns()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter_ns() - t0) / reps * 1e-3
def before():  # what cg_solve does in front of lo_cg_solve_f32 on the general path
    _hip.require_hip(rhs, None); r3 = K._flat(rhs, 2)
    s = desc.c_struct(); ps = pre.c_struct(); prm = K._cg_params(1, 0, 1000, 20, 1e-4, 1e-10, 1e-10, 0)
    K._eigform_due(pre.rs_uses + 1, B)
    ws = _hip.workspace(lib.lo_cg_workspace_bytes(C.byref(s), C.byref(ps), C.byref(prm)), rhs.device)
    x = torch.empty_like(r3); info = _hip.CgInfo()
    return (_hip.ptr(r3), _hip.ptr(x), _hip.ptr(ws), ws.numel(), C.byref(info), _hip.stream_ptr(rhs.device))
info = _hip.CgInfo(); xx = torch.empty_like(rhs)
def after():  # ... and behind it
    ex = _hip.CgPlan(); lib.lo_cg_last_executed(C.byref(ex)); return K._cg_result(xx.reshape(rhs.shape), None, info)
def kernel_us():
    _hip.prof_enable(True)
    for _ in range(50): step()
    torch.cuda.synchronize(); pr = _hip.prof_report(); _hip.prof_enable(False)
    return {k: v[1] / v[0] * 1e3 for k, v in pr.items()}
def host_marks():
    _hip.prof_enable(2)
    for _ in range(400): step()
    torch.cuda.synchronize(); pr = _hip.prof_report(); _hip.prof_enable(False)
    return {k[5:]: v[1] / v[0] * 1e3 for k, v in pr.items() if k.startswith("host:")}
for _ in range(30): step()
print(f"(c) python before the call   {timeit(before):7.2f} us   (general path; includes the two allocations and lo_cg_workspace_bytes)")
print(f"(b) python after the call    {timeit(after):7.2f} us   (general path)")
has_fast = has_sessions and hasattr(K, "cg_fast_entry") and K.cg_fast_entry(None) == "native"  # (csrc/lo_pyfast.cpp)
for mode in (("general", "session", "native") if has_fast else ("general", "session") if has_sessions else ("general",)):
    if mode == "general": os.environ["LO_CG_NO_SESSION"] = "1"
    else: os.environ.pop("LO_CG_NO_SESSION", None)
    if has_fast: K.cg_fast_entry(mode == "native")  # "session": the ctypes binding of the same entry point
    for _ in range(30): step()
    t, k = timeit(step), kernel_us()
    line = f"{mode:8s} step {t:7.2f} us   kernel {k.get('cg_onchip', float('nan')):7.2f} us   host share {t - k.get('cg_onchip', 0.0):6.2f} us"
    if has_sessions:
        m = host_marks()
        line += "   " + "   ".join(f"{n} {v:5.2f} us" for n, v in sorted(m.items()))
    print(line)
