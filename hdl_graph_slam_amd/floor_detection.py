"""FloorDetectionNodelet::detect (apps/floor_detection_nodelet.cpp:110-238) on the device: height clip -> normal filter -> RANSAC plane ->
acceptance tests, one call into hgs_detect_floor.  The rosparam names and defaults are the nodelet's (:57-63); the constants it hard-codes
(normal k 10, :219; RANSAC distance threshold 0.1, :140; pcl::SampleConsensus' 1000 iterations and probability 0.99) and the seed of the
hypothesis generator are keyword arguments.  Nothing here computes on the CPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .registration import DeviceCloud, RegistrationHIP

REASONS = {L.HGS_FLOOR_DETECTED: "DETECTED", L.HGS_FLOOR_TOO_FEW_POINTS: "TOO_FEW_POINTS", L.HGS_FLOOR_TOO_FEW_INLIERS: "TOO_FEW_INLIERS",
           L.HGS_FLOOR_NOT_VERTICAL: "NOT_VERTICAL"}


def floor_params_from_rosparams(pnh: dict | None = None, **constants) -> L.HgsFloorParams:
    """initialize_params (:56-66) over a dict of private rosparams; `constants`: normal_k, ransac_distance_threshold,
    ransac_max_iterations, ransac_probability, seed."""
    pnh = pnh or {}
    p = L.HgsFloorParams()
    rc = L.lib().hgs_floor_params_default(C.byref(p))
    if rc != L.HGS_OK:
        raise ValueError(f"hgs_floor_params_default -> {L.STATUS.get(rc, rc)}")
    p.tilt_deg = float(pnh.get("tilt_deg", p.tilt_deg))
    p.sensor_height = float(pnh.get("sensor_height", p.sensor_height))
    p.height_clip_range = float(pnh.get("height_clip_range", p.height_clip_range))
    p.floor_pts_thresh = int(pnh.get("floor_pts_thresh", p.floor_pts_thresh))
    p.floor_normal_thresh = float(pnh.get("floor_normal_thresh", p.floor_normal_thresh))
    p.use_normal_filtering = int(bool(pnh.get("use_normal_filtering", bool(p.use_normal_filtering))))
    p.normal_filter_thresh = float(pnh.get("normal_filter_thresh", p.normal_filter_thresh))
    for name, value in constants.items():
        if name not in ("normal_k", "ransac_distance_threshold", "ransac_max_iterations", "ransac_probability", "seed"):
            raise TypeError(f"unknown floor detection constant '{name}'")
        setattr(p, name, value)
    return p


class FloorDetector:
    """detect(cloud) -> the floor's coefficients (float32[4], normal upward) or None, like the nodelet's boost::optional.  `engine`: an
    existing RegistrationHIP whose resident clouds (its prefilter() output: the nodelet's /filtered_points, :44) go in without a download;
    without one the detector creates its own on `device_id`."""

    def __init__(self, pnh: dict | None = None, device_id: int = 0, engine: RegistrationHIP | None = None, **constants):
        self.params = floor_params_from_rosparams(pnh, **constants)
        self._own_engine = engine is None
        if engine is None:
            ep = L.default_params(L.HGS_FAST_GICP)
            ep.device_id = device_id
            engine = RegistrationHIP(ep)
        self.engine = engine
        self.last: L.HgsFloorResult | None = None
        self._filtered: DeviceCloud | None = None
        self._inliers: DeviceCloud | None = None
        self.last_batch: list = []                  # the records of the last detect_batch
        self._batch_filtered: list = []
        self._batch_inliers: list = []

    def _drop_clouds(self):
        for c in (self._filtered, self._inliers, *self._batch_filtered, *self._batch_inliers):
            if c is not None:
                c.close()
        self._filtered = self._inliers = None
        self._batch_filtered, self._batch_inliers = [], []

    def detect(self, cloud) -> np.ndarray | None:
        e = self.engine
        own = not isinstance(cloud, DeviceCloud)
        dc = e.upload(cloud) if own else cloud
        self._drop_clouds()
        res = L.HgsFloorResult()
        f, i = C.c_void_p(), C.c_void_p()
        try:
            e._check(L.lib().hgs_detect_floor(e._h, dc._h, C.byref(self.params), C.byref(res), C.byref(f), C.byref(i)))
        finally:
            if own:
                dc.close()
        self.last = res
        self._filtered = DeviceCloud._adopt(e, f) if f.value else None
        self._inliers = DeviceCloud._adopt(e, i) if i.value else None
        return np.array(res.coeffs, dtype=np.float32) if res.detected else None

    def detect_batch(self, clouds) -> list:
        """`detect` of several clouds in ONE device batch (hgs_detect_floor_batch): the sweeps of one sweep time, or of a replayed run, as
        prefilter_batch returned them.  Returns one entry per cloud — float32[4] or None — each bit for bit what detect(clouds[i]) returns.  Every
        entry of `clouds` is a DeviceCloud or a host array (uploaded for the call).  The records are kept as `last_batch`, the clouds behind
        filtered_points(i) and floor_points(i)."""
        e = self.engine
        n = len(clouds)
        self._drop_clouds()
        uploaded = []
        try:
            dcs = []
            for c in clouds:
                if not isinstance(c, DeviceCloud):
                    c = e.upload(c)
                    uploaded.append(c)
                dcs.append(c)
            arr = (C.c_void_p * max(n, 1))(*[c._h.value for c in dcs])
            res = (L.HgsFloorResult * max(n, 1))()
            f, i = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
            e._check(L.lib().hgs_detect_floor_batch(e._h, arr, n, C.byref(self.params), res, f, i))
        finally:
            for c in uploaded:
                c.close()
        self.last_batch = [res[k] for k in range(n)]
        self._batch_filtered = [DeviceCloud._adopt(e, C.c_void_p(f[k])) if f[k] else None for k in range(n)]
        self._batch_inliers = [DeviceCloud._adopt(e, C.c_void_p(i[k])) if i[k] else None for k in range(n)]
        return [np.array(r.coeffs, dtype=np.float32) if r.detected else None for r in self.last_batch]

    def batch_stats(self) -> dict:
        """hgs_debug_floor_batch_stats of the engine's last detect_batch: clouds, ransac_clouds, ransac_rounds, readbacks."""
        v = [C.c_int32() for _ in range(4)]
        self.engine._check(L.lib().hgs_debug_floor_batch_stats(self.engine._h, *[C.byref(x) for x in v]))
        return dict(zip(("clouds", "ransac_clouds", "ransac_rounds", "readbacks"), (x.value for x in v)))

    @property
    def reason(self) -> str | None:
        return None if self.last is None else REASONS.get(self.last.reason, str(self.last.reason))

    def filtered_points(self, i: int | None = None) -> np.ndarray | None:
        """What floor_filtered_pub publishes (:127-130): the RANSAC input, downloaded on demand (i: of cloud i of the last detect_batch)."""
        c = self._filtered if i is None else self._batch_filtered[i]
        return None if c is None else c.download()

    def floor_points(self, i: int | None = None) -> np.ndarray | None:
        """What floor_points_pub publishes (:168-177): the model's inliers (None when no floor was detected; i: of cloud i of the last detect_batch)."""
        c = self._inliers if i is None else self._batch_inliers[i]
        return None if c is None else c.download()

    # ---- stage hooks (tests)
    def debug_filter(self, cloud: DeviceCloud):
        n = cloud.size
        k1, k2, nrm = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 3))
        vp = C.c_void_p
        self.engine._check(L.lib().hgs_debug_floor_filter(self.engine._h, cloud._h, C.byref(self.params), k1.ctypes.data_as(vp), k2.ctypes.data_as(vp),
                                                          nrm.ctypes.data_as(vp)))
        return k1.astype(bool), k2.astype(bool), nrm

    def debug_ransac_counts(self, cloud: DeviceCloud, i0: int, n: int):
        counts, planes = np.zeros(n, np.int32), np.zeros((n, 4))
        vp = C.c_void_p
        self.engine._check(L.lib().hgs_debug_floor_ransac_counts(self.engine._h, cloud._h, C.byref(self.params), i0, n, counts.ctypes.data_as(vp),
                                                                 planes.ctypes.data_as(vp)))
        return counts, planes

    def close(self):
        self._drop_clouds()
        if self._own_engine and self.engine is not None:
            self.engine.close()
        self.engine = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
