#!/usr/bin/env python3
"""S sweeps through the prefilter as S separate hgs_prefilter_framed calls against ONE hgs_prefilter_batch.

--config kitti (the default):
  * raw HDL-64E sweeps (~119 k points, workloads.make_odometry_stream) through the KITTI launch file's prefilter (hdl_graph_slam_kitti.launch:27-33:
    distance 0.1-100 m, VoxelGrid 0.25 m, RadiusOutlierRemoval 0.5 m / 2), without and with a gyro sample and a mount matrix per sweep;
  * the odometry nodelet's VoxelGrid-only downsample (odometry.make_downsample, 0.1 m) on sweeps of ~15 k points (every 8th return of the same sweeps).
--config nodelet: the outlier removals that need a search tree per sweep, on the same raw sweeps:
  * the prefiltering nodelet's own defaults (apps/prefiltering_nodelet.cpp:52-96: distance 1-100 m, VoxelGrid 0.1 m, StatisticalOutlierRemoval 20 / 1.0);
  * RadiusOutlierRemoval 0.8 m / 2 behind the distance filter, without a voxel grid.
  With --ab-tree a third column: the batch with the engine option "prefilter_batch_tree" = 0 (the sweeps one after the other inside the call).

All columns run in one process, alternating, host call to host return (the clouds of a call are released outside the clock).  Every shape gets an engine
of its own: an engine keeps up to six freed cloud blocks for reuse, and the blocks one shape leaves behind do not fit the next shape's clouds — with one
engine for all shapes, every cloud of a later shape was a hipMalloc and a hipFree in both columns (RADIUS without a grid behind the STATISTICAL shape,
S = 2: 0.77 | 0.87 ms instead of 0.56 | 0.41).

    python scripts/prefilter_batch_timing.py [--config kitti|nodelet] [--ab-tree] [reps] [S ...]

Prints one line per shape: p50 and p10 - p90 of every column in milliseconds, batch / separate, whether the batch's p90 lies below the separate calls' p10,
and whether all outputs are identical bits."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdl_graph_slam_amd import _lib as L, synth, workloads  # noqa: E402
from hdl_graph_slam_amd.registration import RegistrationHIP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=("kitti", "nodelet"), default="kitti")
ap.add_argument("--ab-tree", action="store_true", help="also time the batch under prefilter_batch_tree = 0")
ap.add_argument("reps", nargs="?", type=int, default=30)
ap.add_argument("S", nargs="*", type=int)
args = ap.parse_args()
reps, SS = args.reps, args.S or [1, 2, 4, 8]


def pct(t):
    t = 1e3 * np.asarray(t)
    return float(np.percentile(t, 50)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def records(clouds):
    out = [c.download().tobytes() for c in clouds]
    for c in clouds:
        c.close()
    return out


def race(*columns):
    """columns[0] = the separate calls, columns[1] = the batch, further columns = variants of the batch."""
    times, same = [[] for _ in columns], True
    for rep in range(reps + 3):                     # (the first three size the buffers)
        first = None
        for k, run in enumerate(columns):
            t0 = time.perf_counter()
            clouds = run()
            t1 = time.perf_counter()
            if rep < 4:
                rec = records(clouds)
                first = rec if k == 0 else first
                same = same and rec == first
            else:
                for c in clouds:
                    c.close()
            if rep >= 3:
                times[k].append(t1 - t0)
    p = [pct(t) for t in times]
    cells = " | ".join(f"{v:.3f} ({lo:.3f} - {hi:.3f})" for v, lo, hi in p)
    return f"{cells} | {p[1][0] / p[0][0]:.2f} | {'yes' if p[1][2] < p[0][1] else 'no'} | {'equal' if same else 'MISMATCH'} |"


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
nodelet = params(use_distance_filter=1, distance_near_thresh=1.0, distance_far_thresh=100.0, downsample_method=L.HGS_DOWNSAMPLE_VOXELGRID, downsample_resolution=0.1,
                 outlier_removal_method=L.HGS_OUTLIER_STATISTICAL, statistical_mean_k=20, statistical_stddev=1.0)
radius_tree = params(use_distance_filter=1, distance_near_thresh=1.0, distance_far_thresh=100.0, downsample_method=L.HGS_DOWNSAMPLE_NONE,
                     outlier_removal_method=L.HGS_OUTLIER_RADIUS, radius_radius=0.8, radius_min_neighbors=2)
shapes = {"kitti": (("KITTI prefilter, raw HDL-64E sweeps", raw, kitti, False), ("KITTI prefilter, gyro sample and mount per sweep", raw, kitti, True),
                    ("odometry VoxelGrid 0.1 m", small, odometry, False)),
          "nodelet": (("nodelet default prefilter (VoxelGrid 0.1 m, STATISTICAL 20 / 1.0), raw HDL-64E sweeps", raw, nodelet, False),
                      ("RADIUS 0.8 m / 2 without a voxel grid, raw HDL-64E sweeps", raw, radius_tree, False))}[args.config]
for title, sweeps, p, framed in shapes:
    reg = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
    print(f"\n{title}: {min(map(len, sweeps))}-{max(map(len, sweeps))} points per sweep; reps {reps}")
    extra = " the batch, prefilter_batch_tree = 0 ms |" if args.ab_tree else ""
    print(f"| S | S x hgs_prefilter_framed ms, p50 (p10 - p90) | one hgs_prefilter_batch ms |{extra} batch / separate | p90 < p10 | bits |")
    print("|---|---|---|---|---|---|" + ("---|" if args.ab_tree else ""))
    for S in SS:
        ws = gyro[:S] if framed else [None] * S
        Ts = mount[:S] if framed else [None] * S

        def separate():
            return [reg.prefilter(sweeps[i], p, imu_angular_velocity=ws[i], scan_period=0.1, base_link_transform=Ts[i]) for i in range(S)]

        def batch():
            return reg.prefilter_batch(sweeps[:S], p, imu_angular_velocities=ws, scan_periods=0.1, base_link_transforms=Ts)

        def batch_each():
            reg.set_option("prefilter_batch_tree", 0)
            try:
                return batch()
            finally:
                reg.set_option("prefilter_batch_tree", 1)
        print(f"| {S} | " + race(*((separate, batch, batch_each) if args.ab_tree else (separate, batch))), flush=True)
    reg.close()
