#!/usr/bin/env python3
"""Floor detection (hgs_detect_floor) timings on one GPU; prints one JSON line.  Input: the KITTI-launch shape — one HDL-64E sweep
(synth.make_pair("HDL-64E", 0), raw) through the device prefilter with the KITTI launch file's settings (VOXELGRID 0.25 m, RADIUS 0.5 / 2), the
result resident; detect() on it with the nodelet's defaults, normal filtering on and off:
  * detect_p50_ms / detect_p90_ms: host wall clock around FloorDetector.detect over --reps calls, one seed per call (the RANSAC path differs by seed);
  * ransac_iterations: mean / max over those calls; gpu_ms: the PREFILTER stage's GPU time of one call from hgs_profile_read."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hdl_graph_slam_amd import FloorDetector, synth, _lib as L  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sensor-height", type=float, default=2.0)
    a = ap.parse_args()
    raw = synth.make_pair("HDL-64E", 0)[0]
    reg = select_registration_method({"registration_method": "FAST_GICP"})
    pp = L.HgsPrefilterParams()
    L.lib().hgs_prefilter_params_default(pp)
    pp.downsample_resolution, pp.outlier_removal_method, pp.radius_radius, pp.radius_min_neighbors = 0.25, L.HGS_OUTLIER_RADIUS, 0.5, 2
    sweep = reg.prefilter(raw, pp)
    out = {"raw_points": int(len(raw)), "prefiltered_points": int(sweep.size)}
    for nf in (True, False):
        fd = FloorDetector({"use_normal_filtering": nf, "sensor_height": a.sensor_height}, engine=reg)
        for _ in range(5):
            fd.detect(sweep)
        times, iters, found = [], [], 0
        for seed in range(a.reps):
            fd.params.seed = seed
            t0 = time.perf_counter()
            co = fd.detect(sweep)
            times.append((time.perf_counter() - t0) * 1e3)
            iters.append(fd.last.ransac_iterations)
            found += co is not None
        reg.profile_enable(True)
        reg.profile_read(reset=True)
        fd.detect(sweep)
        gpu_ms = reg.profile_read(reset=True)["prefilter"][0]
        reg.profile_enable(False)
        key = "normal_filtering_on" if nf else "normal_filtering_off"
        out[key] = {"detect_p50_ms": round(float(np.percentile(times, 50)), 4), "detect_p90_ms": round(float(np.percentile(times, 90)), 4), "gpu_ms": round(gpu_ms, 4),
                    "ransac_iterations_mean": round(float(np.mean(iters)), 2), "ransac_iterations_max": int(np.max(iters)), "detected": found, "calls": a.reps,
                    "n_clipped": int(fd.last.n_clipped), "n_filtered": int(fd.last.n_filtered), "n_inliers": int(fd.last.n_inliers)}
        fd.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
