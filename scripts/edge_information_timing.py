#!/usr/bin/env python3
"""The fitness scores of one graph update's K edges (InformationMatrixCalculator::calc_fitness_score behind flush_keyframe_queue and the loop
step, apps/hdl_graph_slam_nodelet.cpp:235,569) as K x hgs_calc_fitness_score against ONE hgs_calc_fitness_score_batch, host call to host return.
The edges run along a chain of K + 1 keyframes of 10-14 k points: keyframe i + 1 is the tree of edge i, keyframe i its query.

    python scripts/edge_information_timing.py [updates]

cold: every update works on freshly uploaded clouds (what odometry edges are: cloud1 is the NEW keyframe) — the uploads are outside the clock, the
      index and seed-grid builds inside;
warm: the same resident clouds every time, everything cached.
Both columns run in one process, alternating update by update.  Prints p50 and the p10-p90 spread of both per K, and fails if a score differs in a bit."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import synth  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARMUP = 3
KS = (1, 2, 5, 10, 20)
tgt, src, T = synth.make_pair("HDL-64E", 3, downsample=0.2)
rng = np.random.default_rng(7)
base = [tgt, src]
sizes = rng.integers(10000, 14001, max(KS) + 1)
assert min(len(tgt), len(src)) >= 14000, (len(tgt), len(src))
chain = [np.ascontiguousarray(base[i % 2][np.sort(rng.permutation(len(base[i % 2]))[:sizes[i]])]) for i in range(max(KS) + 1)]
# edge i: cloud1 = keyframe i + 1 (the new one), cloud2 = keyframe i; poses a few centimetres off what relates the two scans
rel = [np.asarray((np.linalg.inv(T) if i % 2 == 0 else T) @ synth.pose_matrix(rng.normal(0, 0.03, 3), rng.normal(0, 0.003, 3)), np.float32) for i in range(max(KS))]
reg = select_registration_method({"registration_method": "FAST_GICP"}, device_id=0)
print(f"points per keyframe: {min(len(c) for c in chain)}-{max(len(c) for c in chain)}; updates {reps} (+{WARMUP} unmeasured)")


def singles(dev, K):
    return np.array([reg.calc_fitness_score(dev[i + 1], dev[i], rel[i]) for i in range(K)])


def batch(dev, K):
    return reg.calc_fitness_scores([(dev[i + 1], dev[i], rel[i]) for i in range(K)])


def clock(f, dev, K):
    reg.synchronize()
    t0 = time.perf_counter()
    out = f(dev, K)
    return 1e3 * (time.perf_counter() - t0), out


def upload(K):
    dev = [reg.upload(c) for c in chain[:K + 1]]
    reg.synchronize()
    return dev


def close(dev):
    for c in dev:
        c.close()


def stats(t):
    return float(np.percentile(t, 50)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


print("| state | K edges | K x single: p50 (p10-p90) ms | one batch: p50 (p10-p90) ms | batch / single | scores |")
print("|---|---|---|---|---|---|")
rows = {}
for state in ("cold", "warm"):
    for K in KS:
        t_s, t_b, same = [], [], True
        warm_dev = upload(K) if state == "warm" else None
        for rep in range(reps + WARMUP):
            dev = warm_dev or upload(K)
            ts, a = clock(singles, dev, K)
            if state == "cold":
                close(dev)
                dev = upload(K)
            tb, b = clock(batch, dev, K)
            if state == "cold":
                close(dev)
            same = same and a.tobytes() == b.tobytes()
            if rep >= WARMUP:
                t_s.append(ts), t_b.append(tb)
        if warm_dev:
            close(warm_dev)
        s, b = stats(t_s), stats(t_b)
        rows[(state, K)] = (s, b)
        print(f"| {state} | {K} | {s[0]:.3f} ({s[1]:.3f}-{s[2]:.3f}) | {b[0]:.3f} ({b[1]:.3f}-{b[2]:.3f}) | {b[0] / s[0]:.2f} | {'equal' if same else 'MISMATCH'} |", flush=True)
        assert same, (state, K)
reg.close()
s, b = rows[("cold", 10)]
print(f"K = 10 cold: batch p50 {b[0]:.3f} vs single p50 {s[0]:.3f}; spreads {'do not overlap' if b[2] < s[1] else 'OVERLAP'} (batch p90 {b[2]:.3f}, single p10 {s[1]:.3f})")
for state in ("cold", "warm"):
    s, b = rows[(state, 1)]
    print(f"K = 1 {state}: batch p50 {b[0]:.3f} {'inside' if s[1] <= b[0] <= s[2] else 'OUTSIDE'} the single call's p10-p90 {s[1]:.3f}-{s[2]:.3f}")
