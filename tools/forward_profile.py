#!/usr/bin/env python3
"""Per-position kernel times of the single-inflight forwards in a trace.

Reads the chrome-trace JSON written by tools/trace2chrome.py (plain or
.gz) from a `bench.py --full` run under `rocprofv3 --kernel-trace`. The
run ends with the single-inflight latency phase: one context, one forward
at a time, so the tail of the trace is one kernel sequence repeated with
nothing else on the GPU. This tool finds that period, walks back from the
end for as long as whole forwards repeat it on one queue without
overlapping each other, and prints min / median / max duration (us) per
position in the forward — the uncontended cost of every dispatch.

    python tools/trace2chrome.py out/run_kernel_trace.csv trace.json
    python tools/forward_profile.py trace.json [--name-width 60]
"""
import argparse
import gzip
import json
import statistics


def load_events(path):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        doc = json.load(f)
    ev = doc["traceEvents"] if isinstance(doc, dict) else doc
    ev = [e for e in ev if e.get("ph") == "X"]
    ev.sort(key=lambda e: e["ts"])
    return ev


def find_period(names, min_period=4, max_period=2000, repeats=3):
    """Smallest P such that the last `repeats` * P names repeat with
    period P."""
    n = len(names)
    for p in range(min_period, min(max_period, n // (repeats + 1)) + 1):
        if all(names[n - 1 - k] == names[n - 1 - k - p]
               for k in range(repeats * p)):
            return p
    return None


def single_inflight_forwards(events):
    """Forwards (lists of events) from the end of the trace backwards,
    oldest first."""
    names = [e["name"] for e in events]
    p = find_period(names)
    if p is None:
        raise SystemExit("no repeating forward found at the end of the trace")
    template = names[-p:]
    forwards = []
    end = len(events)
    next_start = float("inf")
    while end - p >= 0:
        chunk = events[end - p:end]
        if [e["name"] for e in chunk] != template:
            break
        if len({(e.get("pid"), e.get("tid")) for e in chunk}) != 1:
            break
        if chunk[-1]["ts"] + chunk[-1]["dur"] > next_start:
            break  # overlaps the forward after it: not single-inflight
        forwards.append(chunk)
        next_start = chunk[0]["ts"]
        end -= p
    forwards.reverse()
    return forwards


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("trace")
    ap.add_argument("--name-width", type=int, default=64)
    args = ap.parse_args()

    fw = single_inflight_forwards(load_events(args.trace))
    p = len(fw[0])
    q = fw[0][0].get("tid")
    print(f"# {args.trace}: {len(fw)} single-inflight forwards on {q}, "
          f"{p} dispatches each")
    w = args.name_width
    print(f"{'pos':>3}  {'kernel':<{w}} {'min':>7} {'med':>7} {'max':>7}")
    med_sum = 0.0
    for i in range(p):
        d = [f[i]["dur"] for f in fw]
        med = statistics.median(d)
        med_sum += med
        print(f"{i + 1:>3}  {fw[0][i]['name'][:w]:<{w}} {min(d):7.1f} "
              f"{med:7.1f} {max(d):7.1f}")
    span = [f[-1]["ts"] + f[-1]["dur"] - f[0]["ts"] for f in fw]
    print(f"{'':>3}  {'sum of medians':<{w}} {'':>7} {med_sum:7.1f}")
    print(f"{'':>3}  {'forward span (first start to last end)':<{w}} "
          f"{min(span):7.1f} {statistics.median(span):7.1f} {max(span):7.1f}")


if __name__ == "__main__":
    main()
