#!/usr/bin/env python3
"""n independent registrations as n separate chains against ONE hgs_align_pairs, for FAST_GICP, FAST_VGICP and NDT_OMP (DIRECT7, resolution 1.0):

  * lock-step odometry: S streams, each a prefiltered sweep (~17 k points) against its keyframe —
    S x (hgs_set_target_cloud + hgs_set_source_cloud + hgs_align) against one hgs_align_pairs without a fitness pass;
  * one graph update's loop detection: K new keyframes, N candidates each, keyframes of ~11 k points —
    K x (hgs_set_target_cloud + hgs_loop_match_batch) against one hgs_align_pairs over the K x N pairs with the fitness pass.

Everything resident: indices, covariances and voxel tables of every cloud exist before the clock starts.  Both columns run in one process,
alternating, host call to host return.

    python scripts/align_pairs_timing.py [reps] [method ...]

Prints one line per shape: p50 and p10 - p90 of both in milliseconds, their ratio, and whether the records are identical bits."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import _lib as L, synth  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
methods = sys.argv[2:] or ["FAST_GICP", "FAST_VGICP", "NDT_OMP"]
REG_FIELDS = ["final_transformation", "converged", "iterations", "error", "lm_tries"]


def pct(t):
    t = 1e3 * np.asarray(t)
    return float(np.percentile(t, 50)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def race(separate, paired, same):
    t_sep, t_pair = [], []
    for rep in range(reps + 3):                     # (the first three build what is missing and warm the buffers up)
        t0 = time.perf_counter()
        a = separate()
        t1 = time.perf_counter()
        b = paired()
        t2 = time.perf_counter()
        if rep >= 3:
            t_sep.append(t1 - t0), t_pair.append(t2 - t1)
    (s, s10, s90), (p, p10, p90) = pct(t_sep), pct(t_pair)
    return f"{s:.3f} ({s10:.3f} - {s90:.3f}) | {p:.3f} ({p10:.3f} - {p90:.3f}) | {p / s:.2f} | {'equal' if same(a, b) else 'MISMATCH'} |"


rng = np.random.default_rng(5)
tgt17, src17, _ = synth.make_pair("HDL-64E", 3, downsample=0.2)
tgt11, src11, _ = synth.make_pair("HDL-64E", 3, downsample=0.25)
for method in methods:
    reg = select_registration_method({"registration_method": method, "reg_resolution": 1.0, "reg_nn_search_method": "DIRECT7"}, device_id=0)
    # ---- S odometry streams in lock-step
    SS = (2, 4, 8)
    kf = [reg.upload(tgt17[rng.permutation(len(tgt17))[: len(tgt17) - 53 * k]]) for k in range(max(SS))]
    sw = [reg.upload(src17[rng.permutation(len(src17))[: len(src17) - 37 * k]]) for k in range(max(SS))]
    og = [np.asarray(synth.pose_matrix(rng.normal(0, 0.05, 3), rng.normal(0, 0.003, 3)), np.float32) for _ in sw]
    print(f"\n{method}: odometry streams, keyframes {kf[-1].size}-{kf[0].size} points, sweeps {sw[-1].size}-{sw[0].size}; reps {reps}")
    print("| S streams | S x (set_target + set_source + align) ms, p50 (p10 - p90) | one hgs_align_pairs ms | paired / separate | bits |")
    print("|---|---|---|---|---|")
    for S in SS:
        def separate():
            out = []
            for i in range(S):
                reg.setInputTarget(kf[i]), reg.setInputSource(sw[i])
                r = reg.align(og[i])
                out.append((bytes(r.final_transformation), r.converged, r.iterations, r.error, r.lm_tries))
            return out

        def paired():
            return reg.align_pairs(kf[:S], sw[:S], og[:S])

        def same(a, b):
            return a == [(b["final_transformation"][i].tobytes(), b["converged"][i], b["iterations"][i], b["error"][i], b["lm_tries"][i]) for i in range(S)]
        print(f"| {S} | " + race(separate, paired, same), flush=True)
    # ---- K new keyframes x N loop candidates, with the fitness pass
    KS, NS = (2, 5, 10), (6, 12, 24)
    targets = [reg.upload(tgt11[rng.permutation(len(tgt11))[: len(tgt11) - 53 * k]]) for k in range(max(KS))]
    pool = [reg.upload(src11[rng.permutation(len(src11))[: len(src11) - 37 * k]]) for k in range(max(NS) + max(KS))]
    guess = [np.asarray(synth.pose_matrix(rng.normal(0, 0.15, 3), rng.normal(0, 0.01, 3)), np.float32) for _ in pool]
    print(f"\n{method}: loop candidates, targets {targets[-1].size}-{targets[0].size} points, candidates {pool[-1].size}-{pool[0].size}; reps {reps}")
    print("| K new keyframes | N candidates | K x (set_target + batch) ms, p50 (p10 - p90) | one hgs_align_pairs ms | paired / separate | bits |")
    print("|---|---|---|---|---|---|")
    for K, N in zip(KS, NS):
        def separate():
            out = []
            for g in range(K):
                reg.setInputTarget(targets[g])
                out.append(reg.loop_match_batch(pool[g:g + N], guess[g:g + N])[0])
            return out

        def paired():
            return reg.align_pairs([targets[g] for g in range(K) for _ in range(N)], [c for g in range(K) for c in pool[g:g + N]],
                                   [x for g in range(K) for x in guess[g:g + N]], L.DBL_MAX)

        def same(a, b):
            flat = np.concatenate(a)
            return all(flat[f].tobytes() == b[f].tobytes() for f in REG_FIELDS + ["fitness_score", "num_inliers"])
        print(f"| {K} | {N} | " + race(separate, paired, same), flush=True)
    for c in kf + sw + targets + pool:
        c.close()
    reg.close()
