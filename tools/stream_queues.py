#!/usr/bin/env python3
"""Which hardware queue every stream's kernels ran on, from a rocprofv3 --kernel-trace CSV of bench.py, and where in a
steady-state window no table walk is resident (the companion of tools/pipeline_timeline.py, which prints the spans).
    python tools/stream_queues.py <kernel_trace.csv>
Per stream: the queue ids its kernels carry, launches and busy ms inside a window of four steps, and its kernels by
name.  Then the streams that share a queue, the launch count / grid / stream of every kernel name over the whole trace
(to compare two builds), and the gaps of the union of both walks inside the window."""
import collections
import csv
import re
import sys


def tag(n):
    if "k_msm29" in n:
        return "G1walk" if "G1Acc29" in n else "G2walk"
    m = re.search(r"\b(k_[a-z0-9_]+)", n)
    return m.group(1) if m else n[:24]


rows = list(csv.DictReader(open(sys.argv[1])))
missing = [c for c in ("Queue_Id", "Stream_Id", "Start_Timestamp", "End_Timestamp", "Kernel_Name") if rows and c not in rows[0]]
if not rows or missing:
    sys.exit("not a rocprofv3 kernel trace with queue ids: %s" % (", ".join(missing) or "no rows"))
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), tag(r["Kernel_Name"]), r["Stream_Id"], r["Queue_Id"],
       "x".join(r.get(k, "?") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))) for r in rows]
g1 = [e for e in ev if e[2] == "G1walk" and e[1] - e[0] > 5e6]   # the big batches' walks
if len(g1) < 12:
    sys.exit("fewer than 12 big G1 walks in the trace")
a, b = g1[6][0], g1[10][0]
print("window of four steps: %.2f ms (%.2f ms per step)" % ((b - a) / 1e6, (b - a) / 4e6))
per = collections.defaultdict(lambda: {"q": set(), "n": 0, "busy": 0, "names": collections.Counter()})
for s, e, name, st, q, _ in ev:
    if e > a and s < b:
        p = per[st]
        p["q"].add(q)
        p["n"] += 1
        p["busy"] += min(e, b) - max(s, a)
        p["names"][name] += 1
byq = collections.defaultdict(list)
for st, p in sorted(per.items(), key=lambda kv: int(kv[0]) if kv[0].isdigit() else 0):
    print("stream %-3s queue %-8s launches %4d busy %7.2f ms  %s" % (
        st, ",".join(sorted(p["q"])), p["n"], p["busy"] / 1e6, " ".join("%s:%d" % kv for kv in p["names"].most_common(8))))
    for q in p["q"]:
        byq[q].append(st)
for q, sts in sorted(byq.items()):
    print("queue %-3s carries stream(s) %s%s" % (q, ", ".join(sts), "   <-- shared" if len(sts) > 1 else ""))
walks = sorted((max(s, a), min(e, b)) for s, e, name, *_ in ev if name in ("G1walk", "G2walk") and e > a and s < b)
gaps, end = [], a
for s, e in walks:
    if s > end:
        gaps.append((end, s))
    end = max(end, e)
if end < b:
    gaps.append((end, b))
print("no walk resident: %.2f ms of the window in %d gap(s): %s" % (
    sum(e - s for s, e in gaps) / 1e6, len(gaps), ", ".join("%.2f->%.2f" % ((s - a) / 1e6, (e - a) / 1e6) for s, e in gaps)))
for name in ("G1walk", "G2walk"):
    d = [(e - s) / 1e6 for s, e, n, *_ in ev if n == name and e > a and s < b]
    print("%s mean span in the window: %.2f ms over %d launches" % (name, sum(d) / max(len(d), 1), len(d)))
print("launches / grid / streams per kernel name (whole trace):")
cnt = collections.defaultdict(lambda: [0, set(), set()])
for s, e, name, st, q, grid in ev:
    c = cnt[name]
    c[0] += 1
    c[1].add(grid)
    c[2].add(st)
for name, c in sorted(cnt.items()):
    grids = sorted(c[1])
    print("  %-28s %6d  grids %-40s streams %s" % (name, c[0], ",".join(grids[:3]) + ("..." if len(grids) > 3 else ""),
                                                  ",".join(sorted(c[2]))))
