#!/usr/bin/env python3
"""From a rocprofv3 rocpd database (kernel trace): the busy and idle time of the GPU timeline over the LAST `n` kernels
(the steady state of a repeated call) -- sum of kernel durations, span, and the gaps between consecutive kernels.
`--calls K`: instead, the last K bulk encode calls one by one (a call runs from its first embed_kernel to the lnf_pool_kernel that
matches its last one; calls under 10 ms are skipped) -- span, time some kernel covers, time none does, time two kernels share."""
import sqlite3, sys
db = sqlite3.connect(sys.argv[1])
n = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 2000
if "--calls" in sys.argv:
    K = int(sys.argv[sys.argv.index("--calls") + 1])
    calls, cur, embeds, pools = [], None, 0, 0
    for name, s, e in db.execute("select name, start, end from kernels order by start"):
        if cur is None:
            if "embed_kernel" not in name:
                continue
            cur, embeds, pools = [], 0, 0
        cur.append((s, e))
        embeds += "embed_kernel" in name
        pools += "lnf_pool_kernel" in name
        if pools and pools == embeds:
            calls.append((cur, embeds))
            cur = None
    calls = [c for c in calls if max(e for _, e in c[0]) - c[0][0][0] > 10e6][-K:]
    tot = [0.0] * 4
    for iv, chains in calls:
        t0, hi, covered = iv[0][0], iv[0][0], 0
        for s, e in iv:
            covered += max(0, e - max(s, hi))
            hi = max(hi, e)
        span, busy = hi - t0, sum(e - s for s, e in iv)
        for i, v in enumerate((span, covered, span - covered, busy - covered)):
            tot[i] += v / 1e6 / len(calls)
        print(f"call: {chains} chain(s), {len(iv)} kernels, span {span / 1e6:.3f} ms, covered {covered / 1e6:.3f} ms, uncovered {(span - covered) / 1e6:.3f} ms, "
              f"two kernels at once {(busy - covered) / 1e6:.3f} ms, summed kernel time {busy / 1e6:.3f} ms")
    print(f"mean of {len(calls)} calls: span {tot[0]:.3f} ms, covered {tot[1]:.3f} ms, uncovered {tot[2]:.3f} ms, two kernels at once {tot[3]:.3f} ms")
    sys.exit(0)
rows = list(db.execute("select name, start, end from kernels order by start"))[-n:]
busy = sum(e - s for _, s, e in rows)
span = rows[-1][2] - rows[0][1]
# kernels of two streams overlap (a bulk encode call as two chains): the covered time is the union of the intervals, the gaps are
# what no kernel covers
covered, idle_gaps, hi = 0, [], rows[0][1]
for _, s, e in rows:
    if s > hi:
        idle_gaps.append(s - hi)
    covered += max(0, e - max(s, hi))
    hi = max(hi, e)
print(f"union: covered {covered / 1e6:.3f} ms of span {span / 1e6:.3f} ms (uncovered {(span - covered) / 1e6:.3f} ms in {len(idle_gaps)} gaps), "
      f"two kernels at once for {(busy - covered) / 1e6:.3f} ms")
gaps = [rows[i + 1][1] - rows[i][2] for i in range(len(rows) - 1)]
pos = sorted(g for g in gaps if g > 0)
print(f"kernels {len(rows)}: busy {busy / 1e6:.3f} ms, span {span / 1e6:.3f} ms, idle {100 * (span - busy) / span:.1f} %; "
      f"gap median {pos[len(pos) // 2] / 1e3:.2f} us, p90 {pos[int(len(pos) * 0.9)] / 1e3:.2f} us, max {pos[-1] / 1e3:.1f} us")
