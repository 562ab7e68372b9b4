"""The walk order (lo_resident_order_debug) and the ordered start (lo_resident_start_debug) of k_cg_rspace3 at N = 8192,
R = 32, one column.

  sweep   (default) per B: the launch time (prof scope cg_onchip) and the host time per solve over 100 solves in
          automatic order (consecutive solves walk the batch in opposite directions) and forced forward (every solve
          walks 0 .. B - 1, as before the order was a kernel argument).  Where the gap opens is the evidence on how the
          memory-side cache replaces lines.
  stamps  in-kernel stamps (LO_OC_DEBUG, stderr) of the members given, eight solves each, forward always and then
          alternating forward / reverse; a line in front of every solve names mode, member and direction.

  start   the delta sweep of the ordered start: per B (default 128 256 512) the launch time over 200 solves with the
          start forced on at each delta (whatever the number of rounds and the layout) against the start forced off,
          alternated and repeated; then the automatic rule against off.  deltas=x,y restricts the sweep; LO_MB_N and
          LO_MB_R in the environment replace N = 8192 and R = 32 (other group widths).
  start-stamps MODE DELTA MEMBER ...
          the stamps of `stamps`, alternating walk only, under lo_resident_start_debug(MODE, DELTA): top, top + init
          and "top at" of first-round members are what the start changes.

usage: mb_rs3_order.py [sweep B ...] | [stamps MEMBER ...] | [start [deltas=..] B ...] | [start-stamps MODE DELTA MEMBER ...]
"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("LO_EIGFORM_AFTER_USES", "0")
from linear_operator_amd import _hip, kernels as K

N, R = int(os.environ.get("LO_MB_N", 8192)), int(os.environ.get("LO_MB_R", 32))
dev = torch.device("cuda")


def system(B):
    g = torch.Generator(device=dev); g.manual_seed(3)
    Cm = torch.randn(B, N, R, generator=g, device=dev) / R ** 0.5
    d = torch.rand(B, N, generator=g, device=dev) + 0.5
    rhs = torch.randn(B, N, 1, generator=g, device=dev)
    desc = K.lowrank_diag_descriptor(Cm, d)
    L, perm = K.pivoted_cholesky(K.lowrank_diag_descriptor(Cm, None), 15, contiguous=False)
    pre = K.precond_build(L, d, False, root=Cm, perm=perm)
    solve = lambda: K.cg_solve(desc, rhs, precond=pre, tolerance=1e-4)  # noqa: E731
    for _ in range(5): solve()
    torch.cuda.synchronize()
    return solve


def timed(solve, mode, n=100):
    K.resident_order_debug(mode)
    for _ in range(4): solve()
    torch.cuda.synchronize()
    r0 = K.resident_order_debug()["reversed"]
    _hip.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(n): solve()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) / n * 1e6
    rep = _hip.prof_report(); _hip.prof_enable(False)
    v = rep["cg_onchip"]
    return 1e3 * v[1] / v[0], host, K.resident_order_debug()["reversed"] - r0


def sweep(sizes):
    print("B | operator MB | automatic: launch us, host us/solve, reversed of 100 | forward: launch us, host us/solve | launch gap us")
    for B in sizes:
        solve = system(B)
        rows = [timed(solve, m) for m in (0, 1, 0, 1)]  # (alternated twice: the second pair is printed with the first)
        a = [min(rows[0][i], rows[2][i]) for i in (0, 1)]
        f = [min(rows[1][i], rows[3][i]) for i in (0, 1)]
        print(f"{B} | {B * N * R * 4 / 1e6:.0f} | {rows[0][0]:.1f} {rows[2][0]:.1f}, {rows[0][1]:.1f} {rows[2][1]:.1f}, {rows[0][2]} | "
              f"{rows[1][0]:.1f} {rows[3][0]:.1f}, {rows[1][1]:.1f} {rows[3][1]:.1f} | {f[0] - a[0]:+.1f}", flush=True)
        del solve
        torch.cuda.empty_cache()
    K.resident_order_debug(0)


START_DELTAS = (25, 50, 75, 100, 150, 200, 250, 300)  # 10 ns ticks a step (3 steps at most at N = 8192: up to 9 us)


def start_sweep(sizes, deltas=START_DELTAS, n=200):
    print(f"N = {N}, R = {R}")
    print("B | delta ticks | on: launch us (two repeats) | off: launch us (two repeats) | off - on, lower of each")
    for B in sizes:
        solve = system(B)
        for delta in deltas:
            on, off = [], []
            for _ in range(2):
                K.resident_start_debug(3, delta)
                on.append(timed(solve, 0, n)[0])
                assert K.resident_start_debug()["delta"] == delta
                K.resident_start_debug(1)
                off.append(timed(solve, 0, n)[0])
                assert K.resident_start_debug()["delta"] == 0
            print(f"{B} | {delta} | {on[0]:.2f} {on[1]:.2f} | {off[0]:.2f} {off[1]:.2f} | {min(off) - min(on):+.2f}", flush=True)
        auto, off = [], []
        for _ in range(3):
            K.resident_start_debug(0)
            auto.append(timed(solve, 0, n)[0])
            used = K.resident_start_debug()
            K.resident_start_debug(1)
            off.append(timed(solve, 0, n)[0])
        print(f"{B} | automatic: delta {used['delta']} in {used['ngroups']} groups | "
              f"{' '.join(f'{v:.2f}' for v in auto)} | {' '.join(f'{v:.2f}' for v in off)} | {min(off) - min(auto):+.2f}", flush=True)
        del solve
        torch.cuda.empty_cache()
    K.resident_start_debug(0)


def stamps(members, start=None):
    solve = system(512)
    try:
        if start is not None:
            K.resident_start_debug(*start)
            print(f"## start mode {start[0]} delta {start[1]}", file=sys.stderr, flush=True)
        for name in ("forward_always", "alternating") if start is None else ("alternating",):
            for m in members:
                os.environ["LO_OC_DEBUG"] = str(m)
                for i in range(8):
                    rev = name == "alternating" and i % 2 == 1
                    K.resident_order_debug(2 if rev else 1)
                    print(f"## {name} member {m} {'reverse' if rev else 'forward'}", file=sys.stderr, flush=True)
                    solve()
                    torch.cuda.synchronize()
                os.environ.pop("LO_OC_DEBUG")
                for _ in range(2):  # (keeps the alternation going between members)
                    solve()
    finally:
        os.environ.pop("LO_OC_DEBUG", None)
        K.resident_order_debug(0)
        K.resident_start_debug(0)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "stamps":
        stamps([int(a) for a in args[1:]] or [0, 63, 70, 200, 450, 511])
    elif args and args[0] == "start-stamps":
        stamps([int(a) for a in args[3:]] or [0, 63, 70, 200, 450, 511], start=(int(args[1]), int(args[2])))
    elif args and args[0] == "start":
        opts = {a.split("=")[0]: a.split("=")[1].split(",") for a in args[1:] if "=" in a}
        start_sweep([int(a) for a in args[1:] if "=" not in a] or [128, 256, 512],
                    [int(d) for d in opts["deltas"]] if "deltas" in opts else START_DELTAS)
    else:
        sweep([int(a) for a in args[1:]] or [128, 192, 256, 384, 512])
