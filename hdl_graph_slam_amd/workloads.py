"""Synthetic workloads for BASELINE.json's configs built on hdl_graph_slam_amd.synth."""
from __future__ import annotations

import dataclasses
from concurrent.futures import ThreadPoolExecutor
from typing import List

import numpy as np

from . import synth


@dataclasses.dataclass
class LoopClosureSet:
    target: np.ndarray                # PointXYZI records: the new keyframe (loop_detector.hpp:122)
    candidates: List[np.ndarray]      # PointXYZI records: candidate keyframes (loop_detector.hpp:135)
    T_gt: List[np.ndarray]            # ground-truth candidate -> target transforms (4x4 float64)
    guesses: List[np.ndarray]         # initial guesses: GT + noise, z forced to 0 (loop_detector.hpp:137-142)


def _cast_scans(scene, sensor: str, jobs, downsample: float | None, workers: int) -> List[np.ndarray]:
    """synth.scan (+ voxel_downsample) of every (pose, noise_seed) in `jobs`, in their order.  Every revolution depends on its own pose and
    noise seed only, so `workers` > 1 casts them on that many host threads (numpy releases the GIL inside the ray / box arithmetic) and
    returns the same arrays as the sequential loop."""
    def one(job):
        sc = synth.scan(scene, sensor, job[0], job[1])
        return synth.voxel_downsample(sc, downsample) if downsample else sc
    workers = min(int(workers), len(jobs))
    if workers <= 1:
        return [one(j) for j in jobs]
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(one, jobs))


def make_loop_closure_set(sensor: str, scene_seed: int, n_candidates: int, n_distinct: int = 16, downsample: float | None = None,
                          guess_noise=(0.5, 2.0), spread: float = 20.0, workers: int = 1) -> LoopClosureSet:
    """1 query keyframe + n_candidates candidate keyframes (config 4, SURVEY 8d: candidates at poses within 20 m of the query —
    the gate of launch/hdl_graph_slam.launch:121 —, guesses = ground truth + noise of 0.5 m / 2 deg, z forced to 0 as
    loop_detector.hpp:142 does).

    `n_distinct` scans are ray-cast at poses within `spread` metres of the query along the scene's free corridor; every
    candidate is one of those scans expressed in its own randomly displaced sensor frame, so each has a distinct, known
    ground-truth pose relative to the query.  guess_noise = (RMS translation error in metres, RMS rotation error in degrees).
    `workers`: host threads that ray-cast the scans (the set is the same for every value).
    Rounds 1 and 2 benchmarked a milder set (8 distinct scans within 4 m, noise 0.3 m / 1 deg): MILD_LOOP_SET below."""
    rng = np.random.default_rng(7000 + scene_seed)
    scene = synth.make_scene(scene_seed)
    pose_t = synth.pose_matrix([0.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    poses = []
    for j in range(n_distinct):
        xy = rng.uniform(-spread, spread, 2)
        xy[1] *= 0.3 * min(1.0, 4.0 / spread)   # stay inside the free corridor of the scene (+-1.2 m across)
        poses.append(synth.pose_matrix([xy[0], xy[1], 0.0], np.deg2rad([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-8, 8)])))
    # the scans draw from noise seeds of their own, never from `rng`: casting them after all the poses are drawn leaves every draw where it was
    target, *scans = _cast_scans(scene, sensor, [(pose_t, 1000 + scene_seed)] + [(p, 3000 + 17 * scene_seed + j) for j, p in enumerate(poses)], downsample, workers)
    cands, T_gt, guesses = [], [], []
    for c in range(n_candidates):
        j = c % n_distinct
        D = synth.pose_matrix(rng.uniform(-1.0, 1.0, 3) * [1.0, 1.0, 0.05], np.deg2rad(rng.uniform(-1.0, 1.0, 3) * [1.0, 1.0, 10.0]))
        cloud = synth.transform_cloud(scans[j], np.linalg.inv(D)) if c >= n_distinct else scans[j]
        Tg = np.linalg.inv(pose_t) @ poses[j] @ (D if c >= n_distinct else np.eye(4))
        noise = synth.pose_matrix(rng.normal(0, guess_noise[0] / np.sqrt(3), 3), np.deg2rad(rng.normal(0, guess_noise[1] / np.sqrt(3), 3)))
        g = (Tg @ noise).astype(np.float32)
        g[2, 3] = 0.0
        cands.append(cloud)
        T_gt.append(Tg)
        guesses.append(g)
    return LoopClosureSet(target, cands, T_gt, guesses)


MILD_LOOP_SET = dict(n_distinct=8, guess_noise=(0.3, 1.0), spread=4.0)   # the candidate set of the round-1 / round-2 bench lines


@dataclasses.dataclass
class OdometryStream:
    scans: List[np.ndarray]           # PointXYZI records, one per LiDAR sweep (sensor frame)
    poses: List[np.ndarray]           # ground-truth sensor poses in the world frame (4x4 float64)
    stamps: List[float]


def make_odometry_stream(sensor: str, scene_seed: int, n_scans: int, speed: float = 8.0, rate_hz: float = 10.0, yaw_rate_deg: float = 2.0,
                         downsample: float | None = None, workers: int = 1) -> OdometryStream:
    """A vehicle driving along the free corridor of the synthetic scene at `speed` m/s, one sweep every 1/rate_hz s
    (config 3: KITTI-like 64-beam odometry stream; config 1 with sensor='VLP-16' and a 0.1 m prefilter)."""
    scene = synth.make_scene(scene_seed)
    step = speed / rate_hz
    x0 = -0.5 * step * (n_scans - 1)
    poses, stamps = [], []
    for i in range(n_scans):
        yaw = np.deg2rad(yaw_rate_deg) * np.sin(0.35 * i)
        poses.append(synth.pose_matrix([x0 + step * i, 0.4 * np.sin(0.2 * i), 0.0], [0.0, 0.0, yaw]))
        stamps.append(i / rate_hz)
    scans = _cast_scans(scene, sensor, [(p, 5000 + 31 * scene_seed + i) for i, p in enumerate(poses)], downsample, workers)
    return OdometryStream(scans, poses, stamps)
