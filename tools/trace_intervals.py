"""Gaps between the headline launches in a `rocprofv3 --kernel-trace` run of bench.py: reads every *kernel_trace.csv under
DIR and prints the duration of k_cg_rspace3, the interval from the end of one to the start of the next with no other kernel
in between, and the clearing launches (k_zero_span) per solve."""
import csv, glob, os, sys
import numpy as np
rows = []
for f in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
def stats(a):
    a = np.asarray(a, dtype=np.float64) / 1e3
    return (f"n={a.size} median={np.median(a):.2f} us mean={a.mean():.2f} sd={a.std():.2f} p10={np.percentile(a, 10):.2f} "
            f"p90={np.percentile(a, 90):.2f} min={a.min():.2f} max={a.max():.2f}") if a.size else "none"
rs3 = [(s, e) for s, e, n in rows if "k_cg_rspace3" in n]
zs = sum("k_zero_span" in n for _, _, n in rows)
print(f"kernels {len(rows)}, k_zero_span launches {zs}, k_cg_rspace3 launches {len(rs3)}, ratio {zs / max(1, len(rs3)):.3f}")
print("k_cg_rspace3 duration:", stats([e - s for s, e in rs3]))
gaps = [rows[i + 1][0] - rows[i][1] for i in range(len(rows) - 1)
        if "k_cg_rspace3" in rows[i][2] and "k_cg_rspace3" in rows[i + 1][2]]
print("end k_cg_rspace3 -> start next k_cg_rspace3 (no launch between):", stats(gaps))
