#!/usr/bin/env python3
"""Where the tile kernels sit relative to the k_seed launches in a rocprofv3 kernel trace (the raw *kernel_trace.csv or the
compact file trace_step.sh writes).  Per kernel: dispatches, LDS per workgroup, average and longest duration, the share of
its time that lies inside a k_seed launch, how many dispatches began AND ended inside one launch (they ran beside it), and
how many began inside one and ended within 50 us after its end (they waited for it).
usage: trace_summary.py <trace.csv> [out.csv]"""
import bisect
import csv
import sys


def load(path):
    rows = list(csv.DictReader(open(path)))
    out = []
    for r in rows:
        if "Kernel_Name" in r:
            out.append((r["Kernel_Name"].split("(")[0][:40], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", ""), r.get("LDS_Block_Size", "")))
        else:
            out.append((r["kernel"], int(r["start_ns"]), int(r["end_ns"]), r.get("queue", ""), r.get("lds", "")))
    return out


def main():
    ev = load(sys.argv[1])
    seeds = sorted((s, e) for k, s, e, _, _ in ev if "k_seed<" in k or k.endswith("k_seed"))
    starts = [s for s, _ in seeds]
    per = {}
    for k, s, e, q, lds in ev:
        d = per.setdefault(k, {"n": 0, "sum": 0, "max": 0, "in": 0, "beside": 0, "waited": 0, "lds": lds, "queues": set()})
        d["n"] += 1; d["sum"] += e - s; d["max"] = max(d["max"], e - s); d["queues"].add(q)
        i = bisect.bisect_right(starts, s) - 1
        for j in range(max(i, 0), len(seeds)):
            if seeds[j][0] >= e:
                break
            d["in"] += max(0, min(e, seeds[j][1]) - max(s, seeds[j][0]))
        if i >= 0 and s < seeds[i][1]:
            if e <= seeds[i][1]:
                d["beside"] += 1
            elif e <= seeds[i][1] + 50000:
                d["waited"] += 1
    w = csv.writer(open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout)
    w.writerow(["kernel", "dispatches", "lds", "avg_us", "max_us", "share_inside_seed", "began_and_ended_inside_seed", "began_inside_ended_at_seed_end", "queues"])
    for k, d in sorted(per.items(), key=lambda kv: -kv[1]["sum"]):
        w.writerow([k, d["n"], d["lds"], round(d["sum"] / d["n"] / 1e3, 1), round(d["max"] / 1e3, 1), round(d["in"] / max(d["sum"], 1), 3), d["beside"], d["waited"],
                    " ".join(sorted(d["queues"]))])
    if seeds:
        t0, t1 = min(s for _, s, _, _, _ in ev), max(e for _, _, e, _, _ in ev)
        print("k_seed launches: %d, covering %.1f %% of the traced span" % (len(seeds), 100.0 * sum(e - s for s, e in seeds) / max(t1 - t0, 1)), file=sys.stderr)


if __name__ == "__main__":
    main()
