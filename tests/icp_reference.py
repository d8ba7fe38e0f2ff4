"""TEST-SIDE RESTATEMENT of point-to-point ICP — pcl::IterativeClosestPoint<PointXYZI, PointXYZI> as hdl_graph_slam's factory
configures it (src/hdl_graph_slam/registrations.cpp:57-64: setTransformationEpsilon, setMaximumIterations,
setMaxCorrespondenceDistance, setUseReciprocalCorrespondences; nothing else).  The device engine (HGS_ICP, registration_method
"ICP_HIP"; hdl_graph_slam_amd/csrc/hgs_icp.h) is held to this.

UPSTREAM-KNOWLEDGE (PCL is not vendored with the reference, so this is written from PCL's documented behaviour; functions are cited
by name only):

Setup (IterativeClosestPoint::computeTransformation).  If the guess is not the identity the source is first moved by it, and
final = guess.

Each iteration:
  1. Correspondences (CorrespondenceEstimation::determineCorrespondences / determineReciprocalCorrespondences).  For every finite
     source point p, in input order, moved by the current pose: its exact 1-NN q in the target; the pair is kept when d2 <= max_corr^2.
     With reciprocal correspondences on, q's exact 1-NN in the moved source must also be p itself, again within max_corr^2.
  2. Fewer than 3 pairs (min_number_correspondences_): converged = false, stop, final is kept.
  3. The Umeyama step without scale (TransformationEstimationSVD, which calls Eigen's umeyama on the moved source points and their
     targets): Sigma = (1/n) sum (q - mu_q)(p - mu_p)^T = U S V^T; if det U * det V < 0 the sign of the smallest singular direction is
     flipped; R = U D V^T, t = mu_q - R mu_p.  final = Delta * final, ++iterations.
  4. DefaultConvergenceCriteria::hasConverged, in this order, the first test that fires converges:
       iterations >= max_iterations  — counts as converged (PCL's behaviour; LoopDetector relies on it);
       cos(angle(Delta)) >= rot_thr and |t(Delta)|^2 <= transformation_epsilon, rot_thr = 1 - transformation_epsilon when
         rotation_epsilon <= 0 (hdl never sets it), else rotation_epsilon — a SQUARED translation against an unsquared epsilon (PCL's quirk);
       |mse - mse_prev| < 1e-12, mse = mean d2 of this iteration's pairs, mse_prev starting at DBL_MAX;
       the relative-MSE test is off (euclidean_fitness_epsilon = -DBL_MAX).

Stated deviations of the device engine (and of this restatement, which mirrors its arithmetic):
  * points are moved from the ORIGINAL source by the accumulated pose in double and rounded to float once (PCL transforms its float
    copy of the source step by step); the rounding differs in the last float bit;
  * the reverse search of the reciprocal test looks up T^-1 q in the source's own index instead of a tree rebuilt on the moved source
    every iteration: the same neighbour up to float rounding;
  * the Umeyama step runs in double (PCL instantiates its estimator with Scalar = float);
  * mse_prev starts at DBL_MAX in every registration (PCL keeps it in the criteria object across align() calls of one object);
  * the result's `error` is the last iteration's mse (DBL_MAX if none), `lm_tries` the number of correspondence passes.

Arithmetic: the pose in double; a moved point = (((m0 x + m1 y) + m2 z) + m3) in double, rounded to float (the query that is searched);
exact 1-NN from the CPU oracle's tree (oracle.OracleRegistration.nn_target; the reverse search through a second oracle object whose
target is the source); sums in double."""
from __future__ import annotations

import numpy as np

import oracle as O

DBL_MAX = float(np.finfo(np.float64).max)


def _xyz(cloud) -> np.ndarray:
    if getattr(cloud, "dtype", None) is not None and cloud.dtype.fields is not None:
        return np.stack([cloud["x"], cloud["y"], cloud["z"]], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])


def move(T, pts: np.ndarray) -> np.ndarray:
    """The device's point transform (hgs_icp.h icp_move_point): T (4x4 / 3x4, double) applied to float points, unfused, rounded to float."""
    T = np.asarray(T, np.float64)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    out = np.empty((len(pts), 3), np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def unmove(T, pts: np.ndarray) -> np.ndarray:
    """T^-1 q = R^T (q - t) (hgs_icp.h icp_unmove_point)."""
    T = np.asarray(T, np.float64)
    x, y, z = (pts[:, k].astype(np.float64) - T[k, 3] for k in range(3))
    out = np.empty((len(pts), 3), np.float32)
    for c in range(3):
        out[:, c] = ((T[0, c] * x + T[1, c] * y) + T[2, c] * z).astype(np.float32)
    return out


def umeyama(src: np.ndarray, dst: np.ndarray) -> np.ndarray:
    """Eigen's umeyama(src, dst, with_scaling = false) for row-wise point sets: the 4x4 rigid transform dst ~ R src + t."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    mu_s, mu_d = src.mean(0), dst.mean(0)
    sigma = (dst - mu_d).T @ (src - mu_s) / len(src)
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = mu_d - T[:3, :3] @ mu_s
    return T


def umeyama_from_sums(sums) -> np.ndarray:
    """The same step from the 17 sums of a correspondence pass (pairs, sum p, sum q, sum q p^T row-major, sum d2)."""
    s = np.asarray(sums, np.float64)
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    sigma = s[7:16].reshape(3, 3) / n - np.outer(mq, mp)
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = mq - T[:3, :3] @ mp
    return T


class IcpReference:
    def __init__(self, max_iterations=64, transformation_epsilon=0.01, max_correspondence_distance=2.5, reciprocal=False, rotation_epsilon=0.0):
        self.max_iterations = int(max_iterations)
        self.eps = float(transformation_epsilon)
        self.max_corr2 = float(max_correspondence_distance) * float(max_correspondence_distance)
        self.reciprocal = bool(reciprocal)
        self.rot_thr = rotation_epsilon if rotation_epsilon > 0 else 1.0 - self.eps

    @classmethod
    def from_params(cls, p):
        return cls(p.max_iterations, p.transformation_epsilon, p.max_correspondence_distance, bool(p.reserved), p.rotation_epsilon)

    def setInputTarget(self, cloud):
        self.tgt = _xyz(cloud)
        self._t = O.OracleRegistration(O.default_params(O.HGS_FAST_GICP))
        self._t.setInputTarget(self.tgt)

    def setInputSource(self, cloud):
        xyz = _xyz(cloud)
        self.n_source = len(xyz)
        self.src_idx = np.nonzero(np.isfinite(xyz).all(axis=1))[0].astype(np.int32)
        self.src = xyz[self.src_idx]
        self._s = O.OracleRegistration(O.default_params(O.HGS_FAST_GICP))
        self._s.setInputTarget(xyz)

    def correspond(self, T):
        """One pass at pose T: (source indices, target indices, moved source points, target points, d2) of the kept pairs."""
        p = move(T, self.src)
        j, d2 = self._t.nn_target(p)
        keep = (j >= 0) & (d2.astype(np.float64) <= self.max_corr2)
        if self.reciprocal and keep.any():
            r = unmove(T, self.tgt[j[keep]])
            back, rd2 = self._s.nn_target(r)
            ok = (back == self.src_idx[keep]) & (rd2.astype(np.float64) <= self.max_corr2)
            keep[np.nonzero(keep)[0][~ok]] = False
        return self.src_idx[keep], j[keep], p[keep], self.tgt[j[keep]], d2[keep]

    def correspondences(self, T) -> np.ndarray:
        """Per source point (input order): the target index of its pair or -1 (what hgs_debug_icp_correspond returns)."""
        si, tj, _, _, _ = self.correspond(T)
        out = np.full(self.n_source, -1, np.int32)
        out[si] = tj
        return out

    @staticmethod
    def sums(p, q, d2) -> np.ndarray:
        p64, q64 = p.astype(np.float64), q.astype(np.float64)
        return np.concatenate([[len(p)], p64.sum(0), q64.sum(0), (q64.T @ p64).reshape(9), [d2.astype(np.float64).sum()]])

    def after_pass(self, sums, T, mse_prev, iterations, delta=None, mse=None) -> dict:
        """What follows a correspondence pass (hgs_icp.h icp_after_pass) from the pass's 17 sums and the state (T, mse_prev, iterations):
        fewer than 3 pairs -> not converged, done, state kept; else the Umeyama step (delta, or the step from the sums), T = Delta T,
        ++iterations and DefaultConvergenceCriteria's tests in their order.  align() hands in the step and the mse it has from the pairs themselves."""
        sums = np.asarray(sums, np.float64)
        T = np.asarray(T, np.float64)
        if not sums[0] >= 3:
            return {"T": T, "converged": False, "done": True, "iterations": iterations, "mse": None, "mse_prev": mse_prev}
        D = umeyama_from_sums(sums) if delta is None else delta
        iterations += 1
        mse = float(sums[16] / sums[0]) if mse is None else mse
        converged = iterations >= self.max_iterations
        if not converged:
            cos_angle = 0.5 * (np.trace(D[:3, :3]) - 1.0)
            converged = bool(cos_angle >= self.rot_thr and float(D[:3, 3] @ D[:3, 3]) <= self.eps)
        if not converged:
            converged = abs(mse - mse_prev) < 1e-12
        return {"T": D @ T, "converged": converged, "done": converged, "iterations": iterations, "mse": mse, "mse_prev": mse_prev if converged else mse}

    def align(self, guess=None) -> dict:
        T = np.eye(4) if guess is None else np.asarray(guess, np.float32).astype(np.float64)   # the device receives the guess as float
        mse_prev, mse = DBL_MAX, DBL_MAX
        iterations = passes = 0
        while True:
            _, _, p, q, d2 = self.correspond(T)
            passes += 1
            s = np.zeros(17)
            s[0] = len(p)
            some = len(p) >= 3
            o = self.after_pass(s, T, mse_prev, iterations, delta=umeyama(p, q) if some else None, mse=float(d2.astype(np.float64).mean()) if some else None)
            T, iterations, mse_prev = o["T"], o["iterations"], o["mse_prev"]
            if some:
                mse = o["mse"]
            if o["done"]:
                return {"T": T, "converged": o["converged"], "iterations": iterations, "passes": passes, "mse": mse}
