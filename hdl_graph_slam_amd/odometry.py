"""ScanMatchingOdometry — Python mirror of ScanMatchingOdometryNodelet::matching
(apps/scan_matching_odometry_nodelet.cpp:165-262), the odometry caller of the registration engine: frame-to-keyframe
matching with the previous result as the initial guess and a keyframe switch on translation / rotation / time deltas.

The registration object is anything with the pcl::Registration surface the nodelet uses (setInputTarget,
setInputSource, align, hasConverged, getFinalTransformation): hdl_graph_slam_amd.RegistrationHIP on an MI355X, or the CPU
oracle inside the tests.  ROS plumbing (TF, IMU / robot-odometry guesses, status publishing) is out of scope; the
msf_delta hook is kept as an optional argument because it multiplies into the guess (:210).
"""
from __future__ import annotations

import numpy as np


def make_downsample(registration, downsample_method: str = "VOXELGRID", downsample_resolution: float = 0.1):
    """The downsample filter of the odometry nodelet (scan_matching_odometry_nodelet.cpp:84-104, applied at :147-157).

    VOXELGRID (pcl::VoxelGrid) and APPROX_VOXELGRID (pcl::ApproximateVoxelGrid, :91-96) run on the device through hgs_prefilter
    (distance filter and outlier removal off) and return a RESIDENT cloud, so the sweep is uploaded once and registered in
    place; NONE is the pass-through filter the launch files select for this nodelet."""
    method = downsample_method.upper()
    if method in ("VOXELGRID", "APPROX_VOXELGRID"):
        from . import _lib as L
        import ctypes as C
        p = L.HgsPrefilterParams()
        L.lib().hgs_prefilter_params_default(C.byref(p))
        p.use_distance_filter, p.outlier_removal_method = 0, L.HGS_OUTLIER_NONE
        p.downsample_method = L.HGS_DOWNSAMPLE_VOXELGRID if method == "VOXELGRID" else L.HGS_DOWNSAMPLE_APPROX_VOXELGRID
        p.downsample_resolution = downsample_resolution
        return lambda cloud: registration.prefilter(cloud, p)
    return lambda cloud: cloud   # NONE / unknown -> passthrough (:97-103)


def _rotation_angle(R: np.ndarray) -> float:
    """acos(Eigen::Quaternionf(R).w()) — HALF the rotation angle, exactly what the reference thresholds (:226,243)."""
    tr = float(R[0, 0] + R[1, 1] + R[2, 2])
    w = 0.5 * np.sqrt(max(tr + 1.0, 0.0))
    return float(np.arccos(min(1.0, max(-1.0, w))))


class ScanMatchingOdometry:
    def __init__(self, registration, keyframe_delta_trans: float = 0.25, keyframe_delta_angle: float = 0.15, keyframe_delta_time: float = 1.0,
                 transform_thresholding: bool = False, max_acceptable_trans: float = 1.0, max_acceptable_angle: float = 1.0, downsample=None):
        # defaults: scan_matching_odometry_nodelet.cpp:76-83
        self.registration = registration
        self.keyframe_delta_trans = keyframe_delta_trans
        self.keyframe_delta_angle = keyframe_delta_angle
        self.keyframe_delta_time = keyframe_delta_time
        self.transform_thresholding = transform_thresholding
        self.max_acceptable_trans = max_acceptable_trans
        self.max_acceptable_angle = max_acceptable_angle
        self.downsample = downsample or (lambda cloud: cloud)   # :147-157 (launch files use NONE for this nodelet)
        self.keyframe = None
        self.keyframe_pose = np.eye(4, dtype=np.float32)
        self.keyframe_stamp = 0.0
        self.prev_trans = np.eye(4, dtype=np.float32)
        self.num_keyframes = 0
        self.last_result = None

    def matching(self, stamp: float, cloud, msf_delta=None) -> np.ndarray:
        """Returns odom = keyframe_pose * trans (Eigen::Matrix4f semantics: float32 products)."""
        filtered, guess = self.before_align(stamp, cloud, msf_delta)
        if guess is None:
            self.registration.setInputTarget(self.keyframe)
            return np.eye(4, dtype=np.float32)
        self.registration.setInputSource(filtered)
        result = self.registration.align(guess)                     # :210
        self.last_result = result
        odom, switched = self.after_align(stamp, filtered, bool(result.converged), result.matrix())
        if switched:
            self.registration.setInputTarget(self.keyframe)
        return odom

    # The two halves of matching() around the registration, without a word to the engine: LockstepOdometry runs them per stream around one align_pairs.
    def before_align(self, stamp: float, cloud, msf_delta=None):
        """(filtered cloud, guess); guess None: the first sweep, which has become the keyframe (the caller makes it the target)."""
        if self.keyframe is None:                                   # :166-174
            self.prev_trans = np.eye(4, dtype=np.float32)
            self.keyframe_pose = np.eye(4, dtype=np.float32)
            self.keyframe_stamp = stamp
            self.keyframe = self.downsample(cloud)
            self.num_keyframes = 1
            return self.keyframe, None
        filtered = self.downsample(cloud)                           # :176-177
        guess = self.prev_trans if msf_delta is None else (self.prev_trans @ np.asarray(msf_delta, np.float32)).astype(np.float32)
        return filtered, guess

    def after_align(self, stamp: float, filtered, converged: bool, matrix):
        """The decisions of :214-252 on a registration's outcome: (odom, whether `filtered` has become the keyframe — the caller makes it the target)."""
        if not converged:                                           # :214-218
            return (self.keyframe_pose @ self.prev_trans).astype(np.float32), False
        trans = np.asarray(matrix, np.float32)                      # :220
        odom = (self.keyframe_pose @ trans).astype(np.float32)
        if self.transform_thresholding:                             # :223-233
            delta = (np.linalg.inv(self.prev_trans) @ trans).astype(np.float32)
            dx = float(np.linalg.norm(delta[:3, 3]))
            da = _rotation_angle(delta[:3, :3])
            if dx > self.max_acceptable_trans or da > self.max_acceptable_angle:
                return (self.keyframe_pose @ self.prev_trans).astype(np.float32), False
        self.prev_trans = trans                                     # :236
        delta_trans = float(np.linalg.norm(trans[:3, 3]))           # :241-243
        delta_angle = _rotation_angle(trans[:3, :3])
        delta_time = stamp - self.keyframe_stamp
        if delta_trans > self.keyframe_delta_trans or delta_angle > self.keyframe_delta_angle or delta_time > self.keyframe_delta_time:
            self.keyframe = filtered                                # :245-252
            self.keyframe_pose = odom
            self.keyframe_stamp = stamp
            self.prev_trans = np.eye(4, dtype=np.float32)
            self.num_keyframes += 1
            return odom, True
        return odom, False


class LockstepOdometry:
    """n odometry streams on ONE engine, one device batch per sweep time: the reference runs one ScanMatchingOdometryNodelet per LiDAR, each a
    launch-bound chain per sweep; here the streams that have a keyframe register (keyframe i, filtered sweep i, guess i) in one align_pairs
    (hgs_align_pairs: the engine's own target and source play no part) and then take the per-stream decisions of
    scan_matching_odometry_nodelet.cpp:214-252 unchanged.  A keyframe switch replaces that stream's resident target.  The clouds are resident
    DeviceClouds of `registration` (or host clouds, which are uploaded).

    prefilter_params (an hgs_prefilter_params): `matching` takes the RAW host sweeps and prefilters those of one sweep time in one prefilter_batch
    (hgs_prefilter_batch; base_link_transforms: one sensor -> base_link matrix, or None, per stream) instead of one prefilter call per stream; the
    streams' own `downsample` then stays the identity.  Without it nothing changes.

    floor_detector (a FloorDetector on `registration`; needs prefilter_params): the sweeps prefiltered at one sweep time go through one detect_batch
    (hgs_detect_floor_batch) — three of the reference's launch files run floor detection on /filtered_points next to the odometry.  The coefficients
    are kept as `last_floors` (None for a stream without a sweep or without a floor).  The odoms do not depend on it; without it nothing changes."""

    def __init__(self, registration, n_streams: int, prefilter_params=None, base_link_transforms=None, floor_detector=None, **nodelet_params):
        self.registration = registration
        self.streams = [ScanMatchingOdometry(registration, **nodelet_params) for _ in range(n_streams)]
        self.last_records = None
        self.prefilter_params = prefilter_params
        self.base_link_transforms = [None] * n_streams if base_link_transforms is None else list(base_link_transforms)
        assert len(self.base_link_transforms) == n_streams
        assert floor_detector is None or (prefilter_params is not None and floor_detector.engine is registration)
        self.floor_detector = floor_detector
        self.last_floors = [None] * n_streams

    def _resident(self, cloud):
        return cloud if hasattr(cloud, "_h") else self.registration.upload(cloud)

    def matching(self, stamp: float, clouds, msf_deltas=None):
        """One sweep per stream (None: the stream has none at this time) -> the list of their odom matrices (None where there was no sweep)."""
        assert len(clouds) == len(self.streams)
        if self.prefilter_params is not None:
            have = [i for i, c in enumerate(clouds) if c is not None]
            filtered = self.registration.prefilter_batch([clouds[i] for i in have], self.prefilter_params,
                                                         base_link_transforms=[self.base_link_transforms[i] for i in have])
            clouds = list(clouds)
            for i, f in zip(have, filtered):
                clouds[i] = f
            if self.floor_detector is not None:
                self.last_floors = [None] * len(self.streams)
                for i, co in zip(have, self.floor_detector.detect_batch(filtered)):
                    self.last_floors[i] = co
        odoms = [None] * len(self.streams)
        work = []
        for i, (st, cloud) in enumerate(zip(self.streams, clouds)):
            if cloud is None:
                continue
            filtered, guess = st.before_align(stamp, cloud, None if msf_deltas is None else msf_deltas[i])
            if guess is None:
                st.keyframe = self._resident(st.keyframe)
                odoms[i] = np.eye(4, dtype=np.float32)
            else:
                work.append((i, self._resident(filtered), guess))
        if work:
            rec = self.registration.align_pairs([self.streams[i].keyframe for i, _, _ in work], [f for _, f, _ in work], [g for _, _, g in work])
            self.last_records = rec
            for k, (i, filtered, _) in enumerate(work):
                T = np.array(rec["final_transformation"][k], np.float32).reshape(4, 4).T
                odoms[i], _ = self.streams[i].after_align(stamp, filtered, bool(rec["converged"][k]), T)
        return odoms
