#!/usr/bin/env python3
"""S prefiltered sweeps through floor detection as S separate hgs_detect_floor calls against ONE hgs_detect_floor_batch:

  * HDL-64E sweeps (workloads.make_odometry_stream) behind the device prefilter at VoxelGrid 0.25 m (the KITTI launch file's resolution);
  * VLP-16 sweeps behind the device prefilter at VoxelGrid 0.1 m (the outdoor / indoor launch files' resolution);

both resident (prefilter_batch's output goes in without a download), with the nodelet's defaults, normal filtering on and off.  Both columns run in one
process, alternating, host call to host return (the clouds of a call are released outside the clock).

    python scripts/floor_batch_timing.py [reps] [S ...]

Prints one line per shape: p50 and p10 - p90 of both in milliseconds, their ratio, whether the batch's p90 lies below the separate calls' p10, whether all
records and output clouds are identical bits, and from hgs_debug_floor_batch_stats the RANSAC rounds the batch enqueued and its blocking read-backs (next to
the separate calls' read-backs: 3 per call that enters RANSAC, one more with the normal filter)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import FloorDetector, _lib as L, workloads  # noqa: E402
from hdl_graph_slam_amd.registration import RegistrationHIP  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
SS = [int(x) for x in sys.argv[2:]] or [2, 4, 8, 16]


def pct(t):
    t = 1e3 * np.asarray(t)
    return float(np.percentile(t, 50)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def cloud_bytes(c):
    return None if c is None else c.download().tobytes()


def separate(fd, sweeps):
    """hgs_detect_floor per sweep; returns (record, filtered cloud, inlier cloud or None) per sweep — the caller closes the clouds outside the clock."""
    from hdl_graph_slam_amd.registration import DeviceCloud
    e = fd.engine
    out = []
    for dc in sweeps:
        res = L.HgsFloorResult()
        f, i = C.c_void_p(), C.c_void_p()
        e._check(L.lib().hgs_detect_floor(e._h, dc._h, C.byref(fd.params), C.byref(res), C.byref(f), C.byref(i)))
        out.append((res, DeviceCloud._adopt(e, f), DeviceCloud._adopt(e, i) if i.value else None))
    return out


def race(fd, sweeps):
    S = len(sweeps)
    t_sep, t_bat, same = [], [], True
    stats = {}
    for rep in range(reps + 4):                     # (the first four size the buffers and compare the outputs)
        t0 = time.perf_counter()
        a = separate(fd, sweeps)
        t1 = time.perf_counter()
        if rep < 4:
            ra = [(bytes(r), cloud_bytes(f), cloud_bytes(i)) for r, f, i in a]
        for _, f, i in a:
            f.close()
            if i is not None:
                i.close()
        t2 = time.perf_counter()
        fd.detect_batch(sweeps)
        t3 = time.perf_counter()
        if rep < 4:
            same = same and ra == [(bytes(fd.last_batch[k]), cloud_bytes(fd._batch_filtered[k]), cloud_bytes(fd._batch_inliers[k])) for k in range(S)]
        stats = fd.batch_stats()
        fd._drop_clouds()
        if rep >= 4:
            t_sep.append(t1 - t0), t_bat.append(t3 - t2)
    (s, s10, s90), (p, p10, p90) = pct(t_sep), pct(t_bat)
    detected = sum(r.detected for r in fd.last_batch)
    return (f"{s:.3f} ({s10:.3f} - {s90:.3f}) | {p:.3f} ({p10:.3f} - {p90:.3f}) | {p / s:.2f} | {'yes' if p90 < s10 else 'no'} | "
            f"{'equal' if same else 'MISMATCH'} | {detected}/{S} | {stats['ransac_rounds']} | {stats['readbacks']} |")


def prefilter_params(resolution):
    p = L.HgsPrefilterParams()
    L.lib().hgs_prefilter_params_default(C.byref(p))
    p.downsample_method, p.downsample_resolution, p.outlier_removal_method = L.HGS_DOWNSAMPLE_VOXELGRID, resolution, L.HGS_OUTLIER_NONE
    return p


reg = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
for sensor, resolution in (("HDL-64E", 0.25), ("VLP-16", 0.1)):
    stream = workloads.make_odometry_stream(sensor, 3, max(SS), workers=min(8, max(SS)))
    resident = reg.prefilter_batch([np.ascontiguousarray(s) for s in stream.scans], prefilter_params(resolution))
    for nf in (True, False):
        fd = FloorDetector({"use_normal_filtering": nf}, engine=reg)
        print(f"\n{sensor} behind VoxelGrid {resolution} m, normal filtering {'on' if nf else 'off'}: {min(c.size for c in resident)}-{max(c.size for c in resident)} "
              f"points per sweep; reps {reps}")
        print("| S | S x hgs_detect_floor ms, p50 (p10 - p90) | one hgs_detect_floor_batch ms | batch / separate | p90 < p10 | bits | detected | rounds | read-backs |")
        print("|---|---|---|---|---|---|---|---|---|")
        for S in SS:
            print(f"| {S} | " + race(fd, resident[:S]), flush=True)
        fd.close()
    for c in resident:
        c.close()
reg.close()
