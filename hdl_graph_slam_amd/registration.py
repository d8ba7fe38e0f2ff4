"""pcl::Registration-shaped front-end of the MI355X backend.

Mirrors the surface hdl_graph_slam's callers use on the object returned by select_registration_method
(reference: apps/scan_matching_odometry_nodelet.cpp:172-246,298-335 and
include/hdl_graph_slam/loop_detector.hpp:122-153): setInputTarget / setInputSource / align / hasConverged /
getFinalTransformation / getFitnessScore / getSearchMethodTarget()->nearestKSearch.  Every call goes through the
C-ABI of include/hgs_registration.h into the HIP library; nothing here computes on the CPU."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L


class HgsError(RuntimeError):
    pass


class DeviceCloud:
    """A cloud resident in HBM (hgs_cloud): a KeyFrame::cloud uploaded once and reused as loop-closure candidate."""

    def __init__(self, reg: "RegistrationHIP", cloud: np.ndarray):
        arr, n, stride = L.cloud_args(cloud)
        self._reg = reg
        self._h = C.c_void_p()
        reg._check(L.lib().hgs_cloud_create(reg._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(self._h)))
        self.size = n

    @classmethod
    def _adopt(cls, reg: "RegistrationHIP", handle) -> "DeviceCloud":
        """Wrap an hgs_cloud the library created (hgs_prefilter)."""
        self = cls.__new__(cls)
        self._reg, self._h = reg, handle
        self.size = int(L.lib().hgs_cloud_size(handle))
        return self

    def download(self) -> np.ndarray:
        """The resident cloud as pcl::PointXYZI records (x, y, z, 1, intensity)."""
        from . import synth
        out = np.zeros(self.size, dtype=synth.POINT_XYZI_DTYPE)
        self._reg._check(L.lib().hgs_cloud_download(self._h, out.ctypes.data_as(C.c_void_p), out.dtype.itemsize))
        return out

    @property
    def device_bytes(self) -> int:
        """hgs_cloud_device_bytes: what this keyframe costs while it stays resident (points, index, covariances, voxel tables)."""
        return int(L.lib().hgs_cloud_device_bytes(self._h))

    def invalidate(self):
        L.lib().hgs_cloud_invalidate(self._h)

    def close(self):
        if self._h:
            self._reg._lib.hgs_cloud_destroy(self._h)   # the library that created it
            self._h = C.c_void_p()

    def __del__(self):
        # also after the engine has been closed: hgs_destroy orphans the clouds it created (their device memory goes with the
        # engine) and hgs_cloud_destroy of an orphan only frees the host-side object
        try:
            self.close()
        except Exception:
            pass


class _SearchMethodTarget:
    def __init__(self, reg):
        self._reg = reg

    def nearestKSearch(self, points: np.ndarray, k: int = 1):
        """(indices [n], squared distances [n]) of the exact nearest target point of every query (k must be 1)."""
        if k != 1:
            raise NotImplementedError("the callers only use k = 1 (scan_matching_odometry_nodelet.cpp:316)")
        arr, n, stride = L.cloud_args(points)
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        self._reg._check(L.lib().hgs_nn_target(self._reg._h, arr.ctypes.data_as(C.c_void_p), n, stride, idx.ctypes.data_as(C.c_void_p),
                                               d2.ctypes.data_as(C.c_void_p)))
        return idx, d2


class RegistrationHIP:
    def __init__(self, params: L.HgsParams):
        self.params = params
        self._h = C.c_void_p()
        self._lib = L.lib()
        rc = self._lib.hgs_create(C.byref(params), C.byref(self._h))
        if rc != L.HGS_OK:
            msg = L.lib().hgs_last_error(None)
            raise HgsError(f"hgs_create failed: {L.STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")
        self._result = None
        self._source_n = 0
        self._source_stride = 0
        self._keep = {}
        # measurement / test knobs (A/B scripts, tests that force a code path): HGS_ENGINE_OPTIONS="knn_replay=1,batch_lanes=1" — read HERE, by the
        # test / bench harness; the library itself reads no tuning variable from the environment (include/hgs_registration.h, hgs_debug_set_option)
        for item in filter(None, os.environ.get("HGS_ENGINE_OPTIONS", "").split(",")):
            key, _, value = item.partition("=")
            self.set_option(key.strip(), int(value))

    def set_option(self, key: str, value: int):
        self._check(L.lib().hgs_debug_set_option(self._h, key.encode(), int(value)))

    def lane_plan(self):
        """(lanes, ahead lanes) of the engine's last batch and the streams all engines of this process hold on its device (hgs_debug_lane_plan)."""
        lanes, ahead, streams = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(L.lib().hgs_debug_lane_plan(self._h, C.byref(lanes), C.byref(ahead), C.byref(streams)))
        return lanes.value, ahead.value, streams.value

    def plan_lanes(self, n_problems: int, tiles_per_problem: int, ordered: bool = True, assume_streams: int = -1):
        """(lanes, ahead lanes) a batch of that shape would get on this engine as it is now (hgs_debug_plan_lanes); nothing runs."""
        lanes, ahead = C.c_int32(), C.c_int32()
        self._check(L.lib().hgs_debug_plan_lanes(self._h, int(n_problems), int(tiles_per_problem), int(bool(ordered)), int(assume_streams), C.byref(lanes), C.byref(ahead)))
        return lanes.value, ahead.value

    def batch_order(self):
        """Caller positions in the order the last loop-match batch ran in; empty: the caller's order (hgs_debug_batch_order)."""
        n = C.c_int32()
        self._check(L.lib().hgs_debug_batch_order(self._h, None, 0, C.byref(n)))
        buf = (C.c_int32 * max(1, n.value))()
        self._check(L.lib().hgs_debug_batch_order(self._h, buf, n.value, C.byref(n)))
        return list(buf[:n.value])

    # ---- life cycle
    def close(self):
        if self._h:
            self._lib.hgs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != L.HGS_OK:
            msg = L.lib().hgs_last_error(self._h)
            raise HgsError(f"{L.STATUS.get(rc, rc)}: {msg.decode() if msg else ''}")

    # ---- pcl::Registration surface
    def setInputTarget(self, cloud):
        if isinstance(cloud, DeviceCloud):
            self._keep["t"] = cloud
            self._check(L.lib().hgs_set_target_cloud(self._h, cloud._h))
        else:
            arr, n, stride = L.cloud_args(cloud)
            self._check(L.lib().hgs_set_target(self._h, arr.ctypes.data_as(C.c_void_p), n, stride))

    def setInputSource(self, cloud):
        if isinstance(cloud, DeviceCloud):
            self._keep["s"] = cloud
            self._source_n = cloud.size
            self._check(L.lib().hgs_set_source_cloud(self._h, cloud._h))
        else:
            arr, n, stride = L.cloud_args(cloud)
            self._source_n = n
            self._check(L.lib().hgs_set_source(self._h, arr.ctypes.data_as(C.c_void_p), n, stride))

    def align(self, guess=None, return_cloud: bool = False):
        """registration->align(*aligned, guess). Returns the hgs_result (and the aligned xyz cloud if requested)."""
        g = L.colmajor16(np.eye(4) if guess is None else guess)
        r = L.HgsResult()
        self._check(L.lib().hgs_align(self._h, L.fptr(g), C.byref(r)))
        self._result = r
        if return_cloud:
            return r, self.transformed_source(r.matrix())
        return r

    def transformed_source(self, T) -> np.ndarray:
        out = np.zeros((self._source_n, 4), np.float32)
        g = L.colmajor16(T)
        self._check(L.lib().hgs_transform_source(self._h, L.fptr(g), out.ctypes.data_as(C.c_void_p), 16))
        return out

    def hasConverged(self) -> bool:
        return bool(self._result.converged) if self._result is not None else False

    def getFinalTransformation(self) -> np.ndarray:
        return self._result.matrix() if self._result is not None else np.eye(4, dtype=np.float32)

    def getFitnessScore(self, max_range: float = L.DBL_MAX, T=None) -> float:
        g = L.colmajor16(self.getFinalTransformation() if T is None else T)
        score, ninl = C.c_double(), C.c_uint32()
        self._check(L.lib().hgs_fitness(self._h, L.fptr(g), float(max_range), C.byref(score), C.byref(ninl)))
        self.last_num_inliers = ninl.value
        return score.value

    def getSearchMethodTarget(self) -> _SearchMethodTarget:
        return _SearchMethodTarget(self)

    # ---- device clouds / batch (LoopDetector::matching)
    def upload(self, cloud) -> DeviceCloud:
        return DeviceCloud(self, cloud)

    def prefilter(self, cloud, params=None, imu_angular_velocity=None, scan_period: float = 0.1, base_link_transform=None) -> DeviceCloud:
        """PrefilteringNodelet::cloud_callback (apps/prefiltering_nodelet.cpp:106-136) on the device: [deskewing ->] [transform into
        base_link_frame ->] distance filter -> voxel grid -> outlier removal.  Returns a resident cloud usable as setInputSource / setInputTarget argument.
        imu_angular_velocity: the angular_velocity of the sensor_msgs/Imu sample `select_imu_sample` picks (None = the
        nodelet's empty imu_queue or deskewing off: no deskewing).  base_link_transform: the 4x4 sensor -> base_link matrix the nodelet hands to
        pcl_ros::transformPointCloud (:114-129), in numpy's row-major layout (None = no base_link_frame: no transform)."""
        if params is None:
            params = L.HgsPrefilterParams()
            self._check(L.lib().hgs_prefilter_params_default(C.byref(params)))
        arr, n, stride = L.cloud_args(cloud)
        h = C.c_void_p()
        w = None if imu_angular_velocity is None else np.ascontiguousarray(imu_angular_velocity, np.float64).reshape(3)
        if base_link_transform is not None:
            m = L.colmajor16(base_link_transform)
            self._check(L.lib().hgs_prefilter_framed(self._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(params),
                                                     None if w is None else w.ctypes.data_as(C.c_void_p), float(scan_period), L.fptr(m), C.byref(h)))
        elif w is None:
            self._check(L.lib().hgs_prefilter(self._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(params), C.byref(h)))
        else:
            self._check(L.lib().hgs_prefilter_deskewed(self._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(params), w.ctypes.data_as(C.c_void_p),
                                                       float(scan_period), C.byref(h)))
        return DeviceCloud._adopt(self, h)

    def prefilter_batch(self, clouds, params=None, imu_angular_velocities=None, scan_periods=0.1, base_link_transforms=None) -> list:
        """`prefilter` of several sweeps in one device batch (hgs_prefilter_batch): the S LiDARs of one sweep time, or the next sweeps of a replayed run.
        Returns one resident DeviceCloud per sweep, each bit for bit what prefilter(clouds[i], params, ...) returns.  One parameter set for all sweeps;
        imu_angular_velocities / base_link_transforms: None, or one entry (or None) per sweep; scan_periods: one number, or one per sweep."""
        if params is None:
            params = L.HgsPrefilterParams()
            self._check(L.lib().hgs_prefilter_params_default(C.byref(params)))
        n = len(clouds)
        per = lambda v: [None] * n if v is None else list(v)
        ws, Ts = per(imu_angular_velocities), per(base_link_transforms)
        periods = [float(scan_periods)] * n if np.isscalar(scan_periods) else [float(x) for x in scan_periods]
        assert len(ws) == n and len(Ts) == n and len(periods) == n
        sweeps = (L.HgsPrefilterSweep * max(n, 1))()
        keep = []      # the arrays the pointers in `sweeps` refer to
        for i, cloud in enumerate(clouds):
            arr, m, stride = L.cloud_args(cloud)
            w = None if ws[i] is None else np.ascontiguousarray(ws[i], np.float64).reshape(3)
            T = None if Ts[i] is None else L.colmajor16(Ts[i])
            keep += [arr, w, T]
            sweeps[i].pts, sweeps[i].n, sweeps[i].stride_bytes, sweeps[i].scan_period = arr.ctypes.data, m, stride, periods[i]
            sweeps[i].imu_angular_velocity = None if w is None else w.ctypes.data
            sweeps[i].sensor_to_base = None if T is None else T.ctypes.data
        out = (C.c_void_p * max(n, 1))()
        self._check(L.lib().hgs_prefilter_batch(self._h, sweeps, n, C.byref(params), out))
        return [DeviceCloud._adopt(self, C.c_void_p(out[i])) for i in range(n)]

    def prefilter_batch_stats(self) -> dict:
        """hgs_debug_prefilter_batch_stats of the engine's last prefilter_batch: sweeps, batched, readbacks, index_builds, tree_launches."""
        v = [C.c_int32() for _ in range(5)]
        self._check(L.lib().hgs_debug_prefilter_batch_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("sweeps", "batched", "readbacks", "index_builds", "tree_launches"), (x.value for x in v)))

    def map_cloud(self, keyframes, poses, resolution: float) -> DeviceCloud:
        """MapCloudGenerator::generate (src/hdl_graph_slam/map_cloud_generator.cpp:13-51) over resident keyframe clouds."""
        n = len(keyframes)
        arr = (C.c_void_p * max(n, 1))(*[k._h for k in keyframes])
        P = np.ascontiguousarray(np.stack([L.colmajor16(p) for p in poses]) if n else np.zeros((0, 16), np.float32))
        h = C.c_void_p()
        self._check(L.lib().hgs_map_cloud_generate(self._h, arr, P.ctypes.data_as(C.c_void_p), n, float(resolution), C.byref(h)))
        return DeviceCloud._adopt(self, h)

    def loop_match_batch(self, candidates, guesses, max_range: float = L.DBL_MAX):
        """Register every candidate DeviceCloud against the current target; returns (records ndarray, best index)."""
        n = len(candidates)
        ptrs = (C.c_void_p * max(n, 1))(*[c._h for c in candidates])
        g = np.ascontiguousarray(np.stack([L.colmajor16(T) for T in guesses]) if n else np.zeros((0, 16), np.float32))
        out = np.zeros(n, dtype=L.RESULT_DTYPE)
        best = C.c_int32(-1)
        self._check(L.lib().hgs_loop_match_batch(self._h, ptrs, n, g.ctypes.data_as(C.c_void_p), float(max_range), out.ctypes.data_as(C.c_void_p),
                                                 C.byref(best)))
        return out, best.value

    def loop_match_groups(self, targets, groups, guesses, max_range: float = L.DBL_MAX, return_status: bool = False):
        """The candidates of several new keyframes in one batch (hgs_loop_match_groups; LoopDetector::detect, loop_detector.hpp:57-68):
        groups[g] — a list of DeviceClouds — is registered against targets[g], guesses[g][i] is the guess of groups[g][i].  Returns
        (records of all candidates, group after group; best index per group, -1 = none).  The engine's own target and source stay as they are.
        return_status: do not raise but return (records, best, status) — HGS_ERR_UNSUPPORTED tells the caller to run one batch per target."""
        ng = len(groups)
        offsets = np.zeros(ng + 1, np.uintp)
        offsets[1:] = np.cumsum([len(g) for g in groups])
        n = int(offsets[ng])
        tptr = (C.c_void_p * max(ng, 1))(*[(t._h if t is not None else None) for t in targets])
        cptr = (C.c_void_p * max(n, 1))(*[c._h for g in groups for c in g])
        flat = [L.colmajor16(T) for gg in guesses for T in gg]
        g = np.ascontiguousarray(np.stack(flat) if flat else np.zeros((0, 16), np.float32))
        out = np.zeros(n, dtype=L.RESULT_DTYPE)
        best = np.full(ng, -1, np.int32)
        rc = L.lib().hgs_loop_match_groups(self._h, tptr, ng, offsets.ctypes.data_as(C.c_void_p), cptr, g.ctypes.data_as(C.c_void_p), float(max_range),
                                           out.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p))
        if return_status:
            return out, best, rc
        self._check(rc)
        return out, best

    def align_pairs(self, targets, sources, guesses, max_range=None, return_status: bool = False):
        """n independent registrations in one device batch (hgs_align_pairs), every registration method: sources[i] against targets[i] from
        guesses[i] — resident DeviceClouds, which may repeat in any role.  max_range: getFitnessScore(max_range) behind every registration
        (None: fitness_score NaN, num_inliers 0, as align).  Returns the record array of loop_match_batch, candidate_id = i.  The engine's own
        target and source stay as they are.  return_status: do not raise but return (records, status)."""
        n = len(sources)
        assert len(targets) == n and len(guesses) == n
        tptr = (C.c_void_p * max(n, 1))(*[(t._h if t is not None else None) for t in targets])
        sptr = (C.c_void_p * max(n, 1))(*[(s._h if s is not None else None) for s in sources])
        g = np.ascontiguousarray(np.stack([L.colmajor16(T) for T in guesses]) if n else np.zeros((0, 16), np.float32))
        out = np.zeros(n, dtype=L.RESULT_DTYPE)
        rng = None if max_range is None else C.byref(C.c_double(float(max_range)))
        rc = L.lib().hgs_align_pairs(self._h, tptr, sptr, g.ctypes.data_as(C.c_void_p), rng, n, out.ctypes.data_as(C.c_void_p))
        if return_status:
            return out, rc
        self._check(rc)
        return out

    # ---- sharded batch: one process per GPU, records all-gathered by RCCL on the engine's stream (include/hgs_registration.h)
    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the 128-byte RCCL id every rank passes to comm_init (hand it over with whatever launched the processes)."""
        buf = (C.c_ubyte * 128)()
        rc = L.lib().hgs_comm_get_unique_id(buf)
        if rc != L.HGS_OK:
            raise HgsError(f"hgs_comm_get_unique_id: {L.STATUS.get(rc, rc)}")
        return bytes(buf)

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._check(L.lib().hgs_comm_init(self._h, int(rank), int(world), buf))

    def comm_finalize(self):
        self._check(L.lib().hgs_comm_finalize(self._h))

    def loop_match_batch_sharded(self, candidates, candidate_ids, guesses, n_total: int, max_range: float = L.DBL_MAX, return_status: bool = False):
        """This rank's candidates (DeviceClouds, their positions in the detection's candidate list, their guesses) -> the records of
        ALL n_total candidates in candidate order and the index the sequential rule selects.  Collective over the communicator.
        return_status: do not raise on an error status but return (records, best, status) — a rank whose own share failed has
        still taken part in the exchange and holds the other ranks' records (include/hgs_registration.h)."""
        n = len(candidates)
        ptrs = (C.c_void_p * max(n, 1))(*[c._h for c in candidates])
        ids = np.ascontiguousarray(np.asarray(candidate_ids, np.int32).reshape(-1))
        g = np.ascontiguousarray(np.stack([L.colmajor16(T) for T in guesses]) if n else np.zeros((0, 16), np.float32))
        out = np.zeros(int(n_total), dtype=L.RESULT_DTYPE)
        best = C.c_int32(-1)
        rc = L.lib().hgs_loop_match_batch_sharded(self._h, ptrs, n, ids.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), int(n_total),
                                                  float(max_range), out.ctypes.data_as(C.c_void_p), C.byref(best))
        if return_status:
            return out, best.value, rc
        self._check(rc)
        return out, best.value

    def calc_fitness_score(self, cloud1: DeviceCloud, cloud2: DeviceCloud, relpose, max_range: float = L.DBL_MAX) -> float:
        """InformationMatrixCalculator::calc_fitness_score (src/hdl_graph_slam/information_matrix_calculator.cpp:49-80)."""
        g = L.colmajor16(relpose)
        score = C.c_double()
        self._check(L.lib().hgs_calc_fitness_score(self._h, cloud1._h, cloud2._h, L.fptr(g), float(max_range), C.byref(score)))
        return score.value

    def calc_fitness_scores(self, pairs, max_range: float = L.DBL_MAX, return_inliers: bool = False):
        """Every edge of a graph update in one device batch (hgs_calc_fitness_score_batch; flush_keyframe_queue and the loop step,
        apps/hdl_graph_slam_nodelet.cpp:235,569): `pairs` is a list of (cloud1, cloud2, relpose) — resident DeviceClouds, cloud1 the tree side.
        Returns the scores as a float64 array, each the bits calc_fitness_score gives for that pair (with return_inliers: and the number of points
        behind each mean, uint32)."""
        n = len(pairs)
        p1 = (C.c_void_p * max(n, 1))(*[p[0]._h for p in pairs])
        p2 = (C.c_void_p * max(n, 1))(*[p[1]._h for p in pairs])
        g = np.ascontiguousarray(np.stack([L.colmajor16(p[2]) for p in pairs]) if n else np.zeros((0, 16), np.float32))
        scores, inliers = np.zeros(n, np.float64), np.zeros(n, np.uint32)
        self._check(L.lib().hgs_calc_fitness_score_batch(self._h, p1, p2, g.ctypes.data_as(C.c_void_p), n, float(max_range),
                                                         scores.ctypes.data_as(C.c_void_p), inliers.ctypes.data_as(C.c_void_p)))
        return (scores, inliers) if return_inliers else scores

    # ---- stage-level hooks (parity tests)
    def cloud_seed_grid(self, cloud: DeviceCloud):
        """(table words as uint32, bits) of the cloud's seed grid; an empty array and 0 when it has none (hgs_debug_cloud_seed_grid)."""
        bits, entries = C.c_int32(), C.c_size_t()
        self._check(L.lib().hgs_debug_cloud_seed_grid(self._h, cloud._h, None, 0, C.byref(bits), C.byref(entries)))
        tab = np.zeros(entries.value, np.uint32)
        if entries.value:
            self._check(L.lib().hgs_debug_cloud_seed_grid(self._h, cloud._h, tab.ctypes.data_as(C.c_void_p), entries.value, C.byref(bits), C.byref(entries)))
        return tab, bits.value

    def nn_target(self, q_xyz):
        return self.getSearchMethodTarget().nearestKSearch(q_xyz, 1)

    def target_covariances(self, n_target: int) -> np.ndarray:
        out = np.zeros((n_target, 6), np.float32)
        self._check(L.lib().hgs_debug_target_covariances(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def gicp_linearize(self, T):
        T12 = np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4])
        H, b, e = np.zeros((6, 6)), np.zeros(6), np.zeros(1)
        corr = np.empty(self._source_n, np.int32)
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_gicp_linearize(self._h, T12.ctypes.data_as(vp), H.ctypes.data_as(vp), b.ctypes.data_as(vp), e.ctypes.data_as(vp),
                                                     corr.ctypes.data_as(vp)))
        return H, b, float(e[0]), corr

    def icp_correspond(self, T):
        """One ICP correspondence pass at pose T: the 17 sums (pairs, sum p, sum q, sum q p^T row-major, sum d2) and, per source
        point, the original index of its target point or -1."""
        T12 = np.ascontiguousarray(np.asarray(T, np.float64)[:3, :4])
        sums = np.zeros(17)
        corr = np.empty(self._source_n, np.int32)
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_icp_correspond(self._h, T12.ctypes.data_as(vp), sums.ctypes.data_as(vp), corr.ctypes.data_as(vp)))
        return sums, corr

    def icp_step(self, sums17, T_in=None, mse_prev: float = L.DBL_MAX, iterations_in: int = 0):
        """One ICP control step (k_icp_solve) on the 17 sums of a correspondence pass, from the state (T_in, mse_prev, iterations_in):
        (T_out 4x4 in double, converged, done, iterations, mse).  Needs a source, no target."""
        T12 = np.ascontiguousarray((np.eye(4) if T_in is None else np.asarray(T_in, np.float64))[:3, :4])
        sums = np.ascontiguousarray(sums17, np.float64).reshape(17)
        out, flags, mse = np.zeros((3, 4)), np.zeros(3, np.int32), np.zeros(1)
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_icp_step(self._h, sums.ctypes.data_as(vp), T12.ctypes.data_as(vp), float(mse_prev), int(iterations_in),
                                               out.ctypes.data_as(vp), flags.ctypes.data_as(vp), mse.ctypes.data_as(vp)))
        T = np.eye(4)
        T[:3] = out
        return T, int(flags[0]), int(flags[1]), int(flags[2]), float(mse[0])

    def ndt_cells(self, cap: int = 1 << 20):
        ijk, mean, icov, npts = np.zeros((cap, 3), np.int32), np.zeros((cap, 3)), np.zeros((cap, 6), np.float32), np.zeros(cap, np.int32)
        n = C.c_int32()
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_ndt_cells(self._h, cap, ijk.ctypes.data_as(vp), mean.ctypes.data_as(vp), icov.ctypes.data_as(vp),
                                                npts.ctypes.data_as(vp), C.byref(n)))
        k = min(n.value, cap)
        return ijk[:k].copy(), mean[:k].copy(), icov[:k].copy(), npts[:k].copy()

    def vgicp_voxels(self, cap: int = 1 << 20):
        """The FAST_VGICP target's Gaussian voxel map: (integer voxel coordinates [m, 3], means [m, 3] in double, the stored float covariances
        [m, 6] = xx, xy, xz, yy, yz, zz, points per voxel [m]), in no particular order."""
        ijk, mean, cov, npts = np.zeros((cap, 3), np.int32), np.zeros((cap, 3)), np.zeros((cap, 6), np.float32), np.zeros(cap, np.int32)
        n = C.c_int32()
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_vgicp_voxels(self._h, cap, ijk.ctypes.data_as(vp), mean.ctypes.data_as(vp), cov.ctypes.data_as(vp),
                                                   npts.ctypes.data_as(vp), C.byref(n)))
        k = min(n.value, cap)
        return ijk[:k].copy(), mean[:k].copy(), cov[:k].copy(), npts[:k].copy()

    def ndt_derivatives(self, p6):
        p = np.ascontiguousarray(p6, np.float64)
        s, g, H = np.zeros(1), np.zeros(6), np.zeros((6, 6))
        vp = C.c_void_p
        self._check(L.lib().hgs_debug_ndt_derivatives(self._h, p.ctypes.data_as(vp), s.ctypes.data_as(vp), g.ctypes.data_as(vp), H.ctypes.data_as(vp)))
        return float(s[0]), g, H

    # ---- measurement
    def profile_enable(self, on: bool = True):
        self._check(L.lib().hgs_profile_enable(self._h, int(on)))

    def profile_read(self, reset: bool = True):
        ms = np.zeros(len(L.STAGES))
        cnt = np.zeros(len(L.STAGES), np.uint64)
        self._check(L.lib().hgs_profile_read(self._h, ms.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), int(reset)))
        return {s: (float(m), int(c)) for s, m, c in zip(L.STAGES, ms, cnt)}

    def synchronize(self):
        self._check(L.lib().hgs_synchronize(self._h))


def select_imu_sample(imu_queue, cloud_stamp):
    """The gyro sample PrefilteringNodelet::deskewing uses (apps/prefiltering_nodelet.cpp:206-216): imu_queue is a list of
    (stamp, angular_velocity) in arrival order; the first sample stamped after the cloud, else the newest one; every sample in
    front of the chosen one is dropped from the queue (the chosen one stays).  Returns the angular velocity, or None for an
    empty queue (the cloud then passes undeskewed)."""
    if not imu_queue:
        return None
    loc = 0
    chosen = imu_queue[0]
    while loc < len(imu_queue):
        chosen = imu_queue[loc]
        if imu_queue[loc][0] > cloud_stamp:
            break
        loc += 1
    del imu_queue[:loc]
    return chosen[1]


def select_best(records: np.ndarray) -> int:
    """The sequential selection rule of loop_detector.hpp:146-153 applied to gathered per-candidate records."""
    rec = np.ascontiguousarray(records)
    best = C.c_int32(-1)
    rc = L.lib().hgs_select_best(rec.ctypes.data_as(C.c_void_p), len(rec), C.byref(best))
    if rc != L.HGS_OK:
        raise HgsError(L.STATUS.get(rc, rc))
    return best.value
