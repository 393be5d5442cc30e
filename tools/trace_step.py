#!/usr/bin/env python3
"""Timeline of ONE Newton step from a rocprofv3 --kernel-trace CSV: every launch between two
consecutive k_assemble_kkt launches with its start, duration and the idle gap before it; the
factorisation's own kernels are summarised in one line each.

--handback: instead, the stretch between two steps as bench.py drives them -- every launch from the
end of k_tail_combine to the start of the next step's k_assemble_kkt*, with the idle gap in front
of each; medians over all such stretches of the trace, those that hold k_advance_outer and those
that do not separately (the first `--skip' stretches, default 5, are warm-up and left out)."""
import csv
import glob
import statistics
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
d = args[0]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", ""))
        for r in csv.DictReader(open(f))]
rows.sort()
asm = [i for i, r in enumerate(rows) if r[2].startswith("k_assemble_kkt")]


def handback(skip):
    tails = [i for i, r in enumerate(rows) if r[2].startswith("k_tail_combine")]
    kinds = {}
    for ti in tails:
        nxt = [a for a in asm if a > ti]
        if not nxt:
            continue
        seq, prev_end = [], rows[ti][1]
        for s, e, n in rows[ti + 1:nxt[0] + 1]:
            seq.append((n.split("<")[0][:40], (s - prev_end) / 1e3, (e - s) / 1e3))
            prev_end = max(prev_end, e)
        total = (rows[nxt[0]][0] - rows[ti][1]) / 1e3
        key = tuple(n for n, _, _ in seq)
        kinds.setdefault(key, []).append((seq, total))
    for key, lst in kinds.items():
        lst = lst[skip:] if len(lst) > skip + 2 else lst
        adv = "with" if any(n.startswith("k_advance_outer") for n in key) else "without"
        tot = [t for _, t in lst]
        print(f"stretch {adv} k_advance_outer, {len(lst)} steps: end of k_tail_combine -> start of "
              f"{key[-1]}: median {statistics.median(tot):.1f} us (min {min(tot):.1f}, max {max(tot):.1f})")
        busy = 0.0
        for k, n in enumerate(key):
            gap = statistics.median(s[k][1] for s, _ in lst)
            dur = statistics.median(s[k][2] for s, _ in lst)
            last = k == len(key) - 1
            busy += 0.0 if last else dur
            print(f"    gap {gap:6.1f} us   {'' if last else f'{dur:6.1f} us'}   {n}")
        print(f"    launches in the stretch: {busy:.1f} us busy (medians)")


if "--handback" in sys.argv:
    sk = [a for a in sys.argv if a.startswith("--skip=")]
    handback(int(sk[0].split("=")[1]) if sk else 5)
    sys.exit(0)
a, b = asm[-2], asm[-1]
t0 = rows[a][0]
prev_end = rows[a - 1][1] if a else t0
fact = ("k_chain_update", "k_diag_chain", "k_trsm_ud", "k_trsm_block", "k_update_diag", "k_ldlt_update", "k_update_jobs")
agg = {}
gap_total = 0
print(f"step = {(rows[b][0] - t0) / 1e3:.1f} us, {b - a} launches")
for s, e, n in rows[a:b]:
    gap = s - prev_end
    gap_total += max(gap, 0)
    prev_end = max(prev_end, e)
    if n.startswith(fact):
        k = n.split("<")[0]
        c = agg.setdefault(k, [0, 0, 0])
        c[0] += 1
        c[1] += e - s
        c[2] += max(gap, 0)
    else:
        print(f"{(s - t0) / 1e3:9.1f}  {(e - s) / 1e3:7.1f} us  gap {gap / 1e3:6.1f}  {n[:60]}")
for k, (c, t, g) in agg.items():
    print(f"   {k:20s} x{c:3d}  {t / 1e3:8.1f} us  gaps {g / 1e3:6.1f}")
print(f"idle gaps in the step: {gap_total / 1e3:.1f} us")
