"""One step of the default bench, kernel by kernel: from the last TYPICAL launch of a kernel (default k_gather_poisson_tet4) to the first
`stop` kernel (default k_cg_start) after it: name, start offset, duration, gap to the launch before -- where the iteration-
independent part of a step goes (assembly, value codes, numeric set-up of the multigrid).

A stretch whose dispatches come from more than one hardware queue (the gamg set-up's side chain beside the first cycle) gets a
column with the queue of every dispatch (the trace's Queue_Id, numbered in order of first appearance: 0 is the solver's stream; the
trace's Stream_Id is not used -- rocprofv3 7.2 gave the side stream's dispatches the solver stream's id in some steps and 0 in
others, their queue was always another one), gap_us is the gap to the dispatch before it ON THE SAME QUEUE, and the last line gives
every queue's busy time and how long two of them ran at once.  With one queue the listing is what it always was.

    python tools/trace_phase.py <rocprofv3 csv dir> [first=k_gather_poisson_tet4] [stop=k_cg_start]
"""
import csv
import glob
import gzip
import os
import sys


def _open(f):
    return gzip.open(f, "rt") if f.endswith(".gz") else open(f)


def main():
    d = sys.argv[1]
    first = sys.argv[2] if len(sys.argv) > 2 else "k_gather_poisson_tet4"
    stop = sys.argv[3] if len(sys.argv) > 3 else "k_cg_start"
    rows = []
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) + glob.glob(os.path.join(d, "**", "*kernel_trace.csv.gz"), recursive=True)
    for f in sorted(files):
        for r in csv.DictReader(_open(f)):
            where = r.get("Queue_Id") or "0"
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("void ", "").split("(")[0], where))
    rows.sort()
    idx = [i for i, r in enumerate(rows) if first in r[2]]
    if not idx:
        print("no launch of", first)
        return
    # (the last launch whose duration is within 15 % of the median of that kernel's launches: an outlier -- the first step's
    # variant, a launch that caught the tracer's own work -- does not stand for "a step")
    durs = sorted(rows[i][1] - rows[i][0] for i in idx)
    med = durs[len(durs) // 2]
    typical = [i for i in idx if abs((rows[i][1] - rows[i][0]) - med) <= 0.15 * med]
    i0 = typical[-1] if typical else idx[-1]
    stretch = []
    for r in rows[i0:]:
        stretch.append(r)
        if stop in r[2]:
            break
    t0 = rows[i0][0]
    streams = []
    for r in stretch:
        if r[3] not in streams:
            streams.append(r[3])
    if len(streams) < 2:
        prev_end = rows[i0][0]
        total = 0.0
        print(f"{'kernel':70s} {'start_us':>10s} {'dur_us':>9s} {'gap_us':>8s}")
        for s, e, n, _ in stretch:
            print(f"{n[:70]:70s} {(s - t0) / 1e3:10.1f} {(e - s) / 1e3:9.2f} {(s - prev_end) / 1e3:8.2f}")
            total += (e - s) / 1e3
            prev_end = e
        print(f"busy {total:.1f} us, span {(prev_end - t0) / 1e3:.1f} us")
        return
    prev_end = {}
    busy = {w: 0.0 for w in streams}
    print(f"{'kernel':70s} {'queue':>6s} {'start_us':>10s} {'dur_us':>9s} {'gap_us':>8s}")
    for s, e, n, w in stretch:
        q = streams.index(w)
        gap = f"{(s - prev_end[w]) / 1e3:8.2f}" if w in prev_end else f"{'-':>8s}"          # (a queue's first dispatch: nothing before it)
        print(f"{n[:70]:70s} {q:6d} {(s - t0) / 1e3:10.1f} {(e - s) / 1e3:9.2f} {gap}")
        busy[w] += (e - s) / 1e3
        prev_end[w] = e
    # time during which dispatches of at least two queues were running
    edges = sorted([(s, 1) for s, _, _, _ in stretch] + [(e, -1) for _, e, _, _ in stretch])
    depth, last, both = 0, t0, 0
    for t, step in edges:
        if depth >= 2:
            both += t - last
        depth += step
        last = t
    end = max(e for _, e, _, _ in stretch)
    print("busy " + ", ".join(f"queue {streams.index(w)}: {busy[w]:.1f} us" for w in streams) +
          f"; two queues at once {both / 1e3:.1f} us; span {(end - t0) / 1e3:.1f} us")


if __name__ == "__main__":
    main()
