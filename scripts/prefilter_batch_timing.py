#!/usr/bin/env python3
"""S sweeps through the prefilter as S separate hgs_prefilter_framed calls against ONE hgs_prefilter_batch:

  * raw HDL-64E sweeps (~119 k points, workloads.make_odometry_stream) through the KITTI launch file's prefilter (hdl_graph_slam_kitti.launch:27-33:
    distance 0.1-100 m, VoxelGrid 0.25 m, RadiusOutlierRemoval 0.5 m / 2), without and with a gyro sample and a mount matrix per sweep;
  * the odometry nodelet's VoxelGrid-only downsample (odometry.make_downsample, 0.1 m) on sweeps of ~15 k points (every 8th return of the same sweeps).

Both columns run in one process, alternating, host call to host return (the clouds of a call are released outside the clock).

    python scripts/prefilter_batch_timing.py [reps] [S ...]

Prints one line per shape: p50 and p10 - p90 of both in milliseconds, their ratio, whether the batch's p90 lies below the separate calls' p10, and whether
all outputs are identical bits."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import _lib as L, synth, workloads  # noqa: E402
from hdl_graph_slam_amd.registration import RegistrationHIP  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
SS = [int(x) for x in sys.argv[2:]] or [1, 2, 4, 8]


def pct(t):
    t = 1e3 * np.asarray(t)
    return float(np.percentile(t, 50)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def records(clouds):
    out = [c.download().tobytes() for c in clouds]
    for c in clouds:
        c.close()
    return out


def race(separate, batch):
    t_sep, t_bat, same = [], [], True
    for rep in range(reps + 3):                     # (the first three size the buffers)
        t0 = time.perf_counter()
        a = separate()
        t1 = time.perf_counter()
        ra = records(a) if rep < 4 else [c.close() for c in a]
        t2 = time.perf_counter()
        b = batch()
        t3 = time.perf_counter()
        if rep < 4:
            same = same and ra == records(b)
        else:
            for c in b:
                c.close()
        if rep >= 3:
            t_sep.append(t1 - t0), t_bat.append(t3 - t2)
    (s, s10, s90), (p, p10, p90) = pct(t_sep), pct(t_bat)
    return (f"{s:.3f} ({s10:.3f} - {s90:.3f}) | {p:.3f} ({p10:.3f} - {p90:.3f}) | {p / s:.2f} | {'yes' if p90 < s10 else 'no'} | "
            f"{'equal' if same else 'MISMATCH'} |")


def params(**fields):
    p = L.HgsPrefilterParams()
    L.lib().hgs_prefilter_params_default(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    return p


stream = workloads.make_odometry_stream("HDL-64E", 3, max(SS), workers=min(8, max(SS)))
raw = [np.ascontiguousarray(s) for s in stream.scans]
small = [np.ascontiguousarray(s[::8]) for s in raw]
rng = np.random.default_rng(9)
gyro = [rng.normal(0, 0.3, 3) for _ in raw]
mount = [np.asarray(synth.pose_matrix(rng.normal(0, 0.5, 3), rng.normal(0, 0.05, 3)), np.float32) for _ in raw]
kitti = params(use_distance_filter=1, distance_near_thresh=0.1, distance_far_thresh=100.0, downsample_method=L.HGS_DOWNSAMPLE_VOXELGRID, downsample_resolution=0.25,
               outlier_removal_method=L.HGS_OUTLIER_RADIUS, radius_radius=0.5, radius_min_neighbors=2)
odometry = params(use_distance_filter=0, downsample_method=L.HGS_DOWNSAMPLE_VOXELGRID, downsample_resolution=0.1, outlier_removal_method=L.HGS_OUTLIER_NONE)
reg = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
for title, sweeps, p, framed in (("KITTI prefilter, raw HDL-64E sweeps", raw, kitti, False), ("KITTI prefilter, gyro sample and mount per sweep", raw, kitti, True),
                                 ("odometry VoxelGrid 0.1 m", small, odometry, False)):
    print(f"\n{title}: {min(map(len, sweeps))}-{max(map(len, sweeps))} points per sweep; reps {reps}")
    print("| S | S x hgs_prefilter_framed ms, p50 (p10 - p90) | one hgs_prefilter_batch ms | batch / separate | p90 < p10 | bits |")
    print("|---|---|---|---|---|---|")
    for S in SS:
        ws = gyro[:S] if framed else [None] * S
        Ts = mount[:S] if framed else [None] * S

        def separate():
            return [reg.prefilter(sweeps[i], p, imu_angular_velocity=ws[i], scan_period=0.1, base_link_transform=Ts[i]) for i in range(S)]

        def batch():
            return reg.prefilter_batch(sweeps[:S], p, imu_angular_velocities=ws, scan_periods=0.1, base_link_transforms=Ts)
        print(f"| {S} | " + race(separate, batch), flush=True)
reg.close()
