"""LoopDetector — Python mirror of include/hdl_graph_slam/loop_detector.hpp with the candidate loop
(loop_detector.hpp:135-154) replaced by ONE batched device call, optionally sharded over the GPUs of a node.

Semantics kept from the reference:
  * find_candidates: accumulated-distance and planar-distance gating (loop_detector.hpp:81-109);
  * guess = new_keyframe_estimate^-1 * candidate_estimate with both rotations re-normalised, guess(2,3) = 0 (:137-142);
  * per candidate: align + getFitnessScore(fitness_score_max_range) (:143-146);
  * selection: iterate in candidate order, skip if !converged or score > best_score, ties replace (:147-153);
  * reject if best_score > fitness_score_thresh (:160), else last_edge_accum_distance = new_keyframe.accum_distance (:168).

reg_hip_batch_new_keyframes (default false): detect() hands the candidates of ALL new keyframes of an update (loop_detector.hpp:57-68) to the
device in one grouped call and replays the reference's order on the host (LoopDetector._detect_grouped).
reg_hip_batch_pairs (default false; acts only together with reg_hip_batch_new_keyframes): where the engine refuses the grouped call (NDT_OMP,
FAST_VGICP) the groups are flattened into (new keyframe, candidate) pairs and matched in ONE hgs_align_pairs, the best candidate selected per
group on the host.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence

import numpy as np

from . import _lib as L
from .registration import RegistrationHIP, DeviceCloud, select_best
from .registrations import select_registration_method


@dataclasses.dataclass(eq=False)
class KeyFrame:
    """The fields of hdl_graph_slam::KeyFrame (include/hdl_graph_slam/keyframe.hpp:24-52) the loop detector reads."""
    cloud: np.ndarray                 # PointXYZI records
    estimate: np.ndarray              # node->estimate(): 4x4 float64
    accum_distance: float
    device_cloud: Optional[DeviceCloud] = None   # resident copy (uploaded once, reused for every later detection)
    id: int = -1                      # KeyFrame::id(): the pose-graph node id — the stable identity multi-GPU sharding uses


@dataclasses.dataclass(eq=False)
class Loop:
    key1: KeyFrame         # new keyframe (loop end)
    key2: KeyFrame         # matched candidate (loop begin)
    relative_pose: np.ndarray


def _normalized_rotation(T: np.ndarray) -> np.ndarray:
    """Eigen::Quaterniond(R).normalized().toRotationMatrix(): project onto SO(3) through the quaternion."""
    R = np.asarray(T, np.float64)[:3, :3]
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    w, x, y, z = q / np.linalg.norm(q)
    out = np.array(T, np.float64, copy=True)
    out[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return out


def loop_guess(new_keyframe_estimate: np.ndarray, candidate_estimate: np.ndarray) -> np.ndarray:
    """loop_detector.hpp:137-142."""
    a = _normalized_rotation(new_keyframe_estimate)
    b = _normalized_rotation(candidate_estimate)
    g = (np.linalg.inv(a) @ b).astype(np.float32)
    g[2, 3] = 0.0
    return g


class LoopDetector:
    def __init__(self, pnh, device_id: int = 0, registration: Optional[RegistrationHIP] = None, shard=None):
        get = pnh.get
        self.distance_thresh = float(get("distance_thresh", 5.0))                       # loop_detector.hpp:40
        self.accum_distance_thresh = float(get("accum_distance_thresh", 8.0))           # :41
        self.distance_from_last_edge_thresh = float(get("min_edge_interval", 5.0))      # :42
        self.fitness_score_max_range = float(get("fitness_score_max_range", L.DBL_MAX))  # :44
        self.fitness_score_thresh = float(get("fitness_score_thresh", 0.5))             # :45
        self.registration = registration or select_registration_method(pnh, device_id)  # :47
        self.last_edge_accum_distance = 0.0
        self.shard = shard  # optional hdl_graph_slam_amd.distributed.CandidateShard (multi-GPU)
        self.batch_new_keyframes = bool(get("reg_hip_batch_new_keyframes", False))
        self.batch_pairs = bool(get("reg_hip_batch_pairs", False))
        self.last_detect_grouped = False   # whether the last detect() went through the grouped (or paired) call

    def detect(self, keyframes: Sequence[KeyFrame], new_keyframes: Sequence[KeyFrame]) -> List[Loop]:
        self.last_detect_grouped = False
        if self.batch_new_keyframes and self.shard is None:
            loops = self._detect_grouped(keyframes, new_keyframes)
            if loops is not None:
                self.last_detect_grouped = True
                return loops
        loops = []
        for nk in new_keyframes:
            loop = self.matching(self.find_candidates(keyframes, nk), nk)
            if loop is not None:
                loops.append(loop)
        return loops

    def _detect_grouped(self, keyframes: Sequence[KeyFrame], new_keyframes: Sequence[KeyFrame]) -> Optional[List[Loop]]:
        """detect() with one device call for the whole update.  The only state the sequential loop carries from one new keyframe to the next
        is last_edge_accum_distance, which matching() only ever RAISES (to the accepted keyframe's accum_distance, :168; keyframes arrive in
        order of accumulated distance), and which only enters through the last-edge gate (:83-86):
          1. a new keyframe that fails the gate against the value at entry fails it against every later value: dropped;
          2. the others get their candidates by the two state-free tests (:90-106) and are matched speculatively, all in one grouped call;
          3. the host replays the loop in order: gate against the running value (a keyframe that now fails is skipped, its records are
             discarded — the sequential loop would not have matched it), selection and threshold (:147-168), raise the value on acceptance.
        A record depends on its own target, source and guess only (bitwise), so what the replay reads is what matching() would have read.
        Returns None when the engine does not serve the grouped call (NDT_OMP, FAST_VGICP) and reg_hip_batch_pairs is off: the caller runs the
        sequential loop.  With the key on, the same groups go through one align_pairs — records bitwise per problem, as the grouped call's."""
        entry = self.last_edge_accum_distance
        groups = []
        for nk in new_keyframes:
            if nk.accum_distance - entry < self.distance_from_last_edge_thresh:
                continue
            cands = self._candidates_by_distance(keyframes, nk)
            if cands:
                groups.append((nk, cands))
        if not groups:
            return []
        reg = self.registration
        guesses = [[loop_guess(nk.estimate, c.estimate) for c in cands] for nk, cands in groups]
        records, best, rc = reg.loop_match_groups([self._resident(nk) for nk, _ in groups], [[self._resident(c) for c in cands] for _, cands in groups],
                                                  guesses, self.fitness_score_max_range, return_status=True)
        if rc == L.HGS_ERR_UNSUPPORTED:
            if not self.batch_pairs:
                return None
            records = reg.align_pairs([self._resident(nk) for nk, cands in groups for _ in cands], [self._resident(c) for _, cands in groups for c in cands],
                                      [g for gs in guesses for g in gs], self.fitness_score_max_range)
            best, first = [], 0
            for _, cands in groups:                                                       # candidate_id and best are per group, as the grouped call's
                records["candidate_id"][first:first + len(cands)] = np.arange(len(cands))
                best.append(select_best(records[first:first + len(cands)]))
                first += len(cands)
        else:
            reg._check(rc)
        loops, first = [], 0
        for g, (nk, cands) in enumerate(groups):
            rec = records[first:first + len(cands)]
            first += len(cands)
            if nk.accum_distance - self.last_edge_accum_distance < self.distance_from_last_edge_thresh:
                continue                                                                  # gated by a loop accepted earlier in this update
            self.last_records = rec
            b = int(best[g])
            if b < 0 or float(rec["fitness_score"][b]) > self.fitness_score_thresh:      # :160-163
                continue
            self.last_edge_accum_distance = nk.accum_distance                             # :168
            loops.append(Loop(nk, cands[b], np.array(rec["final_transformation"][b], np.float32).reshape(4, 4).T.copy()))
        return loops

    def find_candidates(self, keyframes: Sequence[KeyFrame], new_keyframe: KeyFrame) -> List[KeyFrame]:
        if new_keyframe.accum_distance - self.last_edge_accum_distance < self.distance_from_last_edge_thresh:
            return []
        return self._candidates_by_distance(keyframes, new_keyframe)

    def _candidates_by_distance(self, keyframes: Sequence[KeyFrame], new_keyframe: KeyFrame) -> List[KeyFrame]:
        """The two tests of find_candidates that read no detector state (loop_detector.hpp:90-106)."""
        out = []
        p2 = np.asarray(new_keyframe.estimate)[:2, 3]
        for k in keyframes:
            if new_keyframe.accum_distance - k.accum_distance < self.accum_distance_thresh:
                continue
            if np.linalg.norm(np.asarray(k.estimate)[:2, 3] - p2) > self.distance_thresh:
                continue
            out.append(k)
        return out

    def _resident(self, kf: KeyFrame) -> DeviceCloud:
        if kf.device_cloud is None:
            kf.device_cloud = self.registration.upload(kf.cloud)
        return kf.device_cloud

    def matching(self, candidates: Sequence[KeyFrame], new_keyframe: KeyFrame) -> Optional[Loop]:
        if not candidates:
            return None
        reg = self.registration
        reg.setInputTarget(self._resident(new_keyframe))                                  # loop_detector.hpp:122
        guesses = [loop_guess(new_keyframe.estimate, c.estimate) for c in candidates]
        if self.shard is not None:
            # shard by the keyframe's id, not by its position in this detection's list: the resident cloud (and its index /
            # covariances) of a keyframe then lives on one rank for good
            from .distributed import owner_of
            ids = [c.id if c.id >= 0 else i for i, c in enumerate(candidates)]
            mine = [owner_of(k, self.shard.world_size) == self.shard.rank for k in ids]
            records, best = self.shard.match(reg, [self._resident(c) if m else None for c, m in zip(candidates, mine)], guesses,
                                             self.fitness_score_max_range, keyframe_ids=ids)
        else:
            records, best = reg.loop_match_batch([self._resident(c) for c in candidates], guesses, self.fitness_score_max_range)
        self.last_records = records
        if best < 0:
            return None
        best_score = float(records["fitness_score"][best])
        if best_score > self.fitness_score_thresh:                                        # :160
            return None
        self.last_edge_accum_distance = new_keyframe.accum_distance                      # :168
        rel = np.array(records["final_transformation"][best], np.float32).reshape(4, 4).T.copy()
        return Loop(new_keyframe, candidates[best], rel)


def sequential_matching(reg, candidates, new_keyframe, fitness_score_max_range=L.DBL_MAX):
    """The reference's own loop (loop_detector.hpp:135-154) driven through the single-registration API; used by tests to
    check that the batched call selects the same candidate with the same pose."""
    reg.setInputTarget(new_keyframe.cloud)
    best_score, best, rel = L.DBL_MAX, -1, None
    for i, c in enumerate(candidates):
        reg.setInputSource(c.cloud)
        r = reg.align(loop_guess(new_keyframe.estimate, c.estimate))
        score = reg.getFitnessScore(fitness_score_max_range)
        if (not reg.hasConverged()) or score > best_score:
            continue
        best_score, best, rel = score, i, reg.getFinalTransformation()
    return best, best_score, rel
