#!/usr/bin/env python3
"""One graph update's loop detection — K new keyframes, N candidates each (LoopDetector::detect, loop_detector.hpp:57-68) — as K x
(hgs_set_target_cloud + hgs_loop_match_batch) against ONE hgs_loop_match_groups.  FAST_GICP, keyframes of ~11 k points (prefiltered sweeps,
the shapes of DESIGN.md section 9 (g)), everything resident: index and covariances of every cloud exist before the clock starts.
Neighbouring new keyframes share most candidates: group g takes candidates g .. g + N - 1 of one pool.

    python scripts/loop_groups_timing.py [reps]

Prints one line per shape: p50 of both in milliseconds per update, their ratio, and whether the records are identical bits."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import synth  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
tgt, src, T = synth.make_pair("HDL-64E", 3, downsample=0.25)
rng = np.random.default_rng(5)
reg = select_registration_method({"registration_method": "FAST_GICP"}, device_id=0)
KS, NS = (2, 5, 10), (6, 12, 24)
targets = [reg.upload(tgt[rng.permutation(len(tgt))[: len(tgt) - 53 * k]]) for k in range(max(KS))]
pool = [reg.upload(src[rng.permutation(len(src))[: len(src) - 37 * k]]) for k in range(max(NS) + max(KS))]
guess = [np.asarray(synth.pose_matrix(rng.normal(0, 0.15, 3), rng.normal(0, 0.01, 3)), np.float32) for _ in pool]
print(f"points per keyframe: targets {targets[-1].size}-{targets[0].size}, candidates {pool[-1].size}-{pool[0].size}; reps {reps}")
print("| K new keyframes | N candidates | K x (set_target + batch) ms | one grouped call ms | grouped / separate | bits |")
print("|---|---|---|---|---|---|")
for K in KS:
    for N in NS:
        groups = [pool[g:g + N] for g in range(K)]
        guesses = [guess[g:g + N] for g in range(K)]

        def separate():
            out = []
            for g in range(K):
                reg.setInputTarget(targets[g])
                out.append(reg.loop_match_batch(groups[g], guesses[g]))
            return out

        def grouped():
            return reg.loop_match_groups(targets[:K], groups, guesses)

        t_sep, t_grp = [], []
        for rep in range(reps + 3):                     # (the first three build what is missing and warm the buffers up)
            t0 = time.perf_counter()
            a = separate()
            t1 = time.perf_counter()
            b = grouped()
            t2 = time.perf_counter()
            if rep >= 3:
                t_sep.append(t1 - t0), t_grp.append(t2 - t1)
        same = b"".join(r.tobytes() for r, _ in a) == b[0].tobytes() and [x for _, x in a] == list(b[1])
        s, g = 1e3 * float(np.median(t_sep)), 1e3 * float(np.median(t_grp))
        print(f"| {K} | {N} | {s:.3f} | {g:.3f} | {g / s:.2f} | {'equal' if same else 'MISMATCH'} |", flush=True)
reg.close()
