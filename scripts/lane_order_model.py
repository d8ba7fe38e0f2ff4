#!/usr/bin/env python3
"""CPU-only reproduction of the iteration table behind the ordered lanes ("Ordered lanes").

    python scripts/lane_order_model.py [--iterations iterations.npy] [--lanes-out lanes.json]

Builds the benchmark's own candidate set (64 HDL-64E candidates of scene seed 0 against one query keyframe), registers every candidate with the CPU
oracle at the launch-file parameters (FAST_GICP), and prints: the sorted iteration counts, the longest problems of each contiguous lane of 16 (the
plain plan), the hint of every candidate (the translation norm of its guess) against its iterations, their correlation, and the lanes of the ordered
plan (stable sort by hint, descending; first half on two ahead lanes, second half on two crowd lanes).  --iterations reads the counts from a file
(bench.py --dump-outputs writes iterations.npy) instead of running the oracle; --lanes-out writes both plans' per-lane iteration lists for
scripts/lane_timeline.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def split(idx, lanes):
    out, b0 = [], 0
    for i in range(lanes):
        n = (len(idx) - b0) // (lanes - i)
        out.append(idx[b0:b0 + n])
        b0 += n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", default="")
    ap.add_argument("--lanes-out", default="")
    ap.add_argument("--candidates", type=int, default=64)
    a = ap.parse_args()
    from hdl_graph_slam_amd import workloads
    B = a.candidates
    wl = workloads.make_loop_closure_set("HDL-64E", scene_seed=0, n_candidates=B, n_distinct=min(16, B), workers=min(16, os.cpu_count() or 1))
    if a.iterations:
        it = np.load(a.iterations).astype(int).reshape(-1)[:B]
    else:
        import oracle as O
        o = O.OracleRegistration(O.default_params(O.HGS_FAST_GICP))
        o.setInputTarget(wl.target)
        it = []
        for c, g in zip(wl.candidates, wl.guesses):
            o.setInputSource(c)
            it.append(int(o.align(g).iterations))
        it = np.array(it)
    dist = np.array([float(np.linalg.norm(np.asarray(g, np.float32)[:3, 3])) for g in wl.guesses])
    print(f"{B} candidates, mean iterations {it.mean():.4f}")
    print("sorted iterations:", " ".join(map(str, sorted(it))))
    print(f"correlation of iterations with the guess's translation norm: {np.corrcoef(it, dist)[0, 1]:.2f}")
    print(f"problems of 13 or more iterations: distances {sorted(np.round(dist[it >= 13], 1))}; largest count below 11 m: {it[dist < 11].max()}")
    order = list(np.argsort(-(dist.astype(np.float32) ** 2), kind="stable"))
    ahead = (B + 1) // 2
    plans = {"plain": split(list(range(B)), 4), "ordered": split(order[:ahead], 2) + split(order[ahead:], 2)}
    for name, lanes in plans.items():
        print(f"\n{name} plan:")
        for n, lane in enumerate(lanes):
            li = sorted(it[lane], reverse=True)
            print(f"  lane {n}: {len(lane)} problems, iterations {' '.join(map(str, li))}")
    if a.lanes_out:
        json.dump({k: [[int(it[i]) for i in lane] for lane in v] for k, v in plans.items()}, open(a.lanes_out, "w"))


if __name__ == "__main__":
    main()
