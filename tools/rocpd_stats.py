"""Kernel summary (launches/step, ms/step, avg us) from a rocprofv3 rocpd sqlite database.
usage: python tools/rocpd_stats.py results.db STEPS|auto [out.md]
STEPS = every optimizer step in the trace (warm-up, capture and bench.py's eager profiling steps included); `auto` counts them from the
trace: one Adam launch per step (the most frequent kernel whose name holds "adam")."""
import sqlite3, sys
db = sqlite3.connect(sys.argv[1])
cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
name = "name" if "name" in cols else cols[0]
rows = db.execute(f"select {name}, count(*), sum(end-start) from kernels group by {name} order by 3 desc").fetchall()
if sys.argv[2] == "auto":
    steps = max((c for n, c, _ in rows if "adam" in n.lower()), default=0)
    if steps == 0:
        sys.exit("rocpd_stats: no Adam launch in the trace to count steps by")
else:
    steps = int(sys.argv[2])
tot = sum(r[2] for r in rows)
lines = [f"Steps in the trace: {steps}" + (" (counted: Adam launches)" if sys.argv[2] == "auto" else ""), "",
         "| kernel | launches/step | ms/step | avg us |", "|---|---|---|---|"]
for n, c, ns in rows[:40]:
    lines.append(f"| `{n[:70]}` | {c/steps:.1f} | {ns/steps/1e6:.3f} | {ns/c/1e3:.1f} |")
lines.append(f"\nGPU-busy total: {tot/steps/1e6:.3f} ms/step")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 3:
    open(sys.argv[3], "w").write(out + "\n")
