#!/usr/bin/env python3
"""The end of a FAST_GICP batch step out of a rocprofv3 --kernel-trace CSV, lane by lane ("Ordered lanes").

    python scripts/lane_timeline.py <..._kernel_trace.csv> [--step -1] [--lane-iterations lanes.json --plan plain|ordered]

A step is the launches between two groups of k_gicp_init kernels (one per lane); a lane is a stream; a round of a lane ends with its k_gicp_decide.
Printed for the chosen step (default: the last): per lane its rounds, when its LM rounds and its fitness pass end, and the latency of its first
eight rounds; the wall time from the first LM launch to the last k_fitness_final; the time during which at most one lane is still iterating.

With --lane-iterations (scripts/lane_order_model.py --lanes-out: the iteration counts of every lane's problems under both plans) the script also
integrates the time during which three or fewer problems are live.  A trace does not say which problems a lane holds, so lanes are matched to
streams by their round counts (the lane with the longest problem is the stream with the most rounds), and a lane's problem counts as live in round
r while r <= its iterations."""
import argparse
import collections
import csv
import json


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--step", type=int, default=-1)
    ap.add_argument("--lane-iterations", default="")
    ap.add_argument("--plan", default="plain", choices=["plain", "ordered"])
    a = ap.parse_args()
    rows = []
    for r in csv.DictReader(open(a.csv)):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("hgs::", "").split("<")[0]
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r["Stream_Id"]))
    rows.sort()
    # steps: a k_gicp_init more than 1 ms after the previous one opens a new step
    inits = [i for i, k in enumerate(rows) if k[2] == "k_gicp_init"]
    starts = [i for n, i in enumerate(inits) if n == 0 or rows[i][0] - rows[inits[n - 1]][0] > 1_000_000]
    s0 = starts[a.step]
    later = [i for i in starts if i > s0]
    seg = rows[s0:later[0]] if later else rows[s0:]
    seg = [k for k in seg if k[2].startswith(("k_gicp_", "k_fitness"))]
    t0 = min(k[0] for k in seg if k[2] == "k_gicp_linearize")
    lanes = collections.OrderedDict()
    for s, e, name, stream in seg:
        L = lanes.setdefault(stream, dict(decide=[], lin=[], fit_end=0, first=s))
        if name == "k_gicp_decide":
            L["decide"].append(e)
        elif name == "k_gicp_linearize":
            L["lin"].append((s, e))
        elif name == "k_fitness_final":
            L["fit_end"] = e
    end = max(L["fit_end"] for L in lanes.values())
    print(f"step {a.step} of {len(starts)}: first LM launch to last k_fitness_final {(end - t0) / 1e3:.1f} us\n")
    print("| stream | rounds | LM rounds end, us | fitness ends, us | latency of rounds 1-8, us | mean of rounds 9.., us | k_gicp_linearize of the last 3 rounds, us |")
    print("|---|---:|---:|---:|---|---:|---|")
    for stream, L in lanes.items():
        ends = [L["lin"][0][0]] + L["decide"]
        lat = [(ends[i + 1] - ends[i]) / 1e3 for i in range(len(ends) - 1)]
        rest = lat[8:]
        print(f"| {stream} | {len(L['decide'])} | {(L['decide'][-1] - t0) / 1e3:.1f} | {(L['fit_end'] - t0) / 1e3:.1f} | {' '.join(f'{x:.0f}' for x in lat[:8])} | "
              f"{(sum(rest) / len(rest) if rest else 0):.1f} | {' '.join(f'{(e - s) / 1e3:.0f}' for s, e in L['lin'][-3:])} |")
    lm_ends = sorted(L["decide"][-1] for L in lanes.values())
    print(f"\nat most one lane still iterating: {(lm_ends[-1] - lm_ends[-2]) / 1e3:.1f} us (from the second-to-last lane's last round to the last lane's)")
    if a.lane_iterations:
        per_lane = json.load(open(a.lane_iterations))[a.plan]
        by_rounds = sorted(lanes.values(), key=lambda L: -len(L["decide"]))
        by_iters = sorted(per_lane, key=lambda it: -max(it))
        events = []  # (time, change of the live count)
        for L, its in zip(by_rounds, by_iters):
            ends = L["decide"]
            events.append((L["lin"][0][0], len(its)))
            for r in range(1, max(its) + 1):          # a problem of r iterations leaves at the end of the lane's round r (the last lane round: at its end)
                gone = sum(1 for x in its if x == r)
                if gone:
                    events.append((ends[min(r, len(ends)) - 1], -gone))
        events.sort()
        live, few, prev = 0, 0, None
        for t, d in events:
            if prev is not None and 0 < live <= 3:
                few += t - prev
            live += d
            prev = t
        print(f"three or fewer problems live: {few / 1e3:.1f} us")


if __name__ == "__main__":
    main()
