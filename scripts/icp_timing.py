#!/usr/bin/env python3
"""ICP_HIP (HGS_ICP) timings on one GPU; prints one JSON line:
  * single_align_p50_ms: hgs_align of the config-2 HDL-32E raw pair (synth.make_pair("HDL-32E", 5), identity guess), warm (both clouds
    resident with their index), p50 over --reps aligns, host wall clock around the call;
  * loop_batch_reg_per_s: a 64-candidate hgs_loop_match_batch (+ getFitnessScore) over bench.py's keyframes (HDL-64E, scene seed 0, raw) against
    one query keyframe, candidates resident, the query re-uploaded per detection (cold target index), registrations per second;
  * per_iteration_ms: the GPU time of one correspondence pass + one control step (profiling stages LINEARIZE + SOLVE) per round of the
    batch, from hgs_profile_read, and the same for the single align."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hdl_graph_slam_amd import synth, workloads  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402


def stage_ms(reg):
    st = reg.profile_read(reset=True)
    return st["linearize"][0] + st["solve"][0], st["linearize"][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch-steps", type=int, default=10)
    ap.add_argument("--reciprocal", action="store_true")
    a = ap.parse_args()
    pnh = {"registration_method": "ICP_HIP", "reg_use_reciprocal_correspondences": a.reciprocal}
    out = {"method": "ICP_HIP", "reciprocal": a.reciprocal}

    # ---- single align, config-2 pair
    tgt, src, T = synth.make_pair("HDL-32E", 5)
    reg = select_registration_method(pnh)
    t_cloud, s_cloud = reg.upload(tgt), reg.upload(src)
    reg.setInputTarget(t_cloud)
    reg.setInputSource(s_cloud)
    for _ in range(5):
        r = reg.align(np.eye(4))
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = reg.align(np.eye(4))
        times.append((time.perf_counter() - t0) * 1e3)
    out["single_points"] = [int(len(tgt)), int(len(src))]
    out["single_align_p50_ms"] = round(float(np.percentile(times, 50)), 4)
    out["single_iterations"] = int(r.iterations)
    out["single_converged"] = int(r.converged)
    reg.profile_enable(True)
    reg.profile_read(reset=True)
    r = reg.align(np.eye(4))
    gpu_ms, rounds = stage_ms(reg)
    reg.profile_enable(False)
    out["single_per_iteration_ms"] = round(gpu_ms / max(rounds, 1), 4)

    # ---- 64-candidate loop-closure batch, bench.py's keyframes
    wl = workloads.make_loop_closure_set("HDL-64E", 0, n_candidates=64)
    breg = select_registration_method(pnh)
    cands = [breg.upload(c) for c in wl.candidates]
    q = breg.upload(wl.target)
    breg.setInputTarget(q)
    rec, best = breg.loop_match_batch(cands, wl.guesses)
    t0 = time.perf_counter()
    for _ in range(a.batch_steps):
        q.invalidate()
        rec, best = breg.loop_match_batch(cands, wl.guesses)
    dt = time.perf_counter() - t0
    out["batch_points_mean"] = int(np.mean([len(c) for c in wl.candidates]))
    out["loop_batch_reg_per_s"] = round(64 * a.batch_steps / dt, 2)
    out["loop_batch_ms"] = round(dt / a.batch_steps * 1e3, 3)
    out["batch_iterations_mean"] = round(float(np.mean(rec["iterations"])), 2)
    out["batch_iterations_max"] = int(np.max(rec["iterations"]))
    out["batch_converged"] = int(np.sum(rec["converged"]))
    out["batch_best"] = int(best)
    breg.profile_enable(True)
    breg.profile_read(reset=True)
    rec, best = breg.loop_match_batch(cands, wl.guesses)
    gpu_ms, rounds = stage_ms(breg)
    breg.profile_enable(False)
    out["batch_per_iteration_ms"] = round(gpu_ms / max(rounds, 1), 4)
    out["batch_rounds"] = rounds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
