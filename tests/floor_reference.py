"""TEST-ONLY restatement, in numpy fp64, of the floor detection hgs_detect_floor implements (include/hgs_registration.h):
FloorDetectionNodelet::detect of apps/floor_detection_nodelet.cpp:110-238 with the stated deviations from PCL.  Nothing here calls the
library under test: the clip, the normals (exact neighbours from oracle.knn or brute force), the hypothesis generator (restated with Python
integers), the counts and the sequential rule are all written out again."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

DETECTED, TOO_FEW_POINTS, TOO_FEW_INLIERS, NOT_VERTICAL = 0, 1, 2, 3
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


@dataclass
class FloorParams:
    tilt_deg: float = 0.0
    sensor_height: float = 2.0
    height_clip_range: float = 1.0
    floor_pts_thresh: int = 512
    floor_normal_thresh: float = 10.0
    use_normal_filtering: bool = True
    normal_filter_thresh: float = 20.0
    normal_k: int = 10
    ransac_distance_threshold: float = 0.1
    ransac_max_iterations: int = 1000
    ransac_probability: float = 0.99
    seed: int = 0


def xyz64(cloud) -> np.ndarray:
    if cloud.dtype.fields is not None:
        return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float64)
    return np.asarray(cloud, np.float32)[:, :3].astype(np.float64)


def xyz32(cloud) -> np.ndarray:
    if cloud.dtype.fields is not None:
        return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)
    return np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])


def direction(p: FloorParams):
    """r = R^-1 e_z = (-sin, 0, cos) of the float tilt angle, as float32 components (z' = r . p)."""
    if p.tilt_deg == 0.0:
        return np.float32(0.0), np.float32(1.0)
    a = float(np.float32(p.tilt_deg * math.pi / 180.0))
    return np.float32(-math.sin(a)), np.float32(math.cos(a))


# ---- step 1: the height clip, in float like PCL's PlaneClipper3D
def clip_flags(p: FloorParams, cloud) -> np.ndarray:
    f = xyz32(cloud)
    rx, rz = direction(p)
    with np.errstate(invalid="ignore", over="ignore"):
        zt = (rx * f[:, 0]).astype(np.float32) + (rz * f[:, 2]).astype(np.float32)
        lo = np.float32(p.sensor_height + p.height_clip_range)
        hi = np.float32(p.sensor_height - p.height_clip_range)
        keep = ((zt + lo).astype(np.float32) >= 0) & ~((zt + hi).astype(np.float32) >= 0)
    return keep & np.isfinite(f).all(1)


def clip_z64(p: FloorParams, cloud) -> np.ndarray:
    """z' in fp64 (the band test of the tilted clip)."""
    f = xyz64(cloud)
    rx, rz = direction(p)
    return float(rx) * f[:, 0] + float(rz) * f[:, 2]


# ---- step 2: normals of the clipped points
@dataclass
class Normals:
    normals: np.ndarray      # [m, 3] unit eigenvector of the smallest eigenvalue
    keep: np.ndarray         # [m] |n . r| > cos(normal_filter_thresh)
    tie: np.ndarray          # [m] the k-th and (k+1)-th neighbour distances tie
    degenerate: np.ndarray   # [m] (l1 - l0) <= 1e-6 l2
    in_band: np.ndarray      # [m] | |n . r| - cos | <= 1e-9


def neighbours(pts32: np.ndarray, k: int):
    """(indices [m, k], tie flags [m]) of the exact k nearest neighbours of every point among the points, itself included."""
    m = len(pts32)
    if m <= k + 1 or m <= 64:
        d = pts32.astype(np.float64)
        d2 = ((d[:, None, :] - d[None, :, :]) ** 2).sum(2)
        order = np.argsort(d2, axis=1, kind="stable")
        kk = min(k, m)
        idx = order[:, :kk]
        tie = np.zeros(m, bool)
        if m > kk:
            rows = np.arange(m)
            tie = d2[rows, order[:, kk - 1]] == d2[rows, order[:, kk]]
        return idx, tie
    import oracle as O
    idx, d2 = O.knn(np.ascontiguousarray(pts32), np.ascontiguousarray(pts32), k + 1)
    d = pts32.astype(np.float64)
    e2 = ((d[idx] - d[:, None, :]) ** 2).sum(2)          # the same neighbours' distances in fp64
    tie = (d2[:, k - 1] == d2[:, k]) | (e2[:, k - 1] == e2[:, k])
    return idx[:, :k], tie


def normals(p: FloorParams, clipped32: np.ndarray) -> Normals:
    m = len(clipped32)
    rx, rz = direction(p)
    r = np.array([float(rx), 0.0, float(rz)])
    cos = math.cos(p.normal_filter_thresh * math.pi / 180.0)
    if m == 0:
        z = np.zeros(0, bool)
        return Normals(np.zeros((0, 3)), z, z, z, z)
    idx, tie = neighbours(clipped32, p.normal_k)
    q = clipped32.astype(np.float64)[idx]                 # [m, k, 3]
    c = q - q.mean(1, keepdims=True)
    cov = np.einsum("mki,mkj->mij", c, c) / idx.shape[1]
    w, v = np.linalg.eigh(cov)                            # ascending
    n = v[:, :, 0]
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    dot = np.abs(n @ r)
    return Normals(n, dot > cos, tie, (w[:, 1] - w[:, 0]) <= 1e-6 * w[:, 2], np.abs(dot - cos) <= 1e-9)


# ---- step 4: the hypothesis generator (a pure function of seed, i, n) and the counts
def mix64(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample3(seed: int, i: int, n: int):
    base = mix64(((seed & 0xFFFFFFFF) << 32) | (i & 0xFFFFFFFF))
    r0, r1, r2 = (mix64((base + (j + 1) * GOLDEN) & M64) for j in range(3))
    a = r0 % n
    b = r1 % (n - 1)
    if b >= a:
        b += 1
    c = r2 % (n - 2)
    lo, hi = min(a, b), max(a, b)
    if c >= lo:
        c += 1
    if c >= hi:
        c += 1
    return a, b, c


def plane3(pts64: np.ndarray, a: int, b: int, c: int):
    p0, p1, p2 = pts64[a], pts64[b], pts64[c]
    u, v = p1 - p0, p2 - p0
    n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    ln = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if not (ln > 0.0) or not math.isfinite(ln):
        return None
    n = n / ln
    return np.array([n[0], n[1], n[2], -((n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2])])


def distances(plane: np.ndarray, pts64: np.ndarray) -> np.ndarray:
    return np.abs(((plane[0] * pts64[:, 0] + plane[1] * pts64[:, 1]) + plane[2] * pts64[:, 2]) + plane[3])


def hypothesis(p: FloorParams, pts64: np.ndarray, i: int):
    """(count, plane[4], near): near = some point lies within 1e-9 of the threshold (the count may then differ by rounding)."""
    n = len(pts64)
    if n < 3:
        return 0, np.zeros(4), False
    pl = plane3(pts64, *sample3(p.seed, i, n))
    if pl is None:
        return 0, np.zeros(4), False
    with np.errstate(invalid="ignore"):
        d = distances(pl, pts64)
        return int((d < p.ransac_distance_threshold).sum()), pl, bool((np.abs(d - p.ransac_distance_threshold) <= 1e-9).any())


@dataclass
class Ransac:
    iterations: int = 0
    best: int = 0
    best_i: int = -1
    plane: np.ndarray = field(default_factory=lambda: np.zeros(4))
    near: bool = False        # a count the rule looked at had a point within 1e-9 of the threshold


def ransac(p: FloorParams, pts64: np.ndarray) -> Ransac:
    """The sequential rule of pcl::RandomSampleConsensus::computeModel over the generator's hypotheses."""
    n = len(pts64)
    out = Ransac()
    k = 1.0
    log_prob = math.log(1.0 - p.ransac_probability)
    eps = float(np.finfo(np.float64).eps)
    i = 0
    while i < k and i < p.ransac_max_iterations:
        count, pl, near = hypothesis(p, pts64, i)
        out.near |= near
        if count > out.best:
            out.best, out.best_i, out.plane = count, i, pl
            w = count / n
            p_no = min(max(1.0 - (w * w) * w, eps), 1.0 - eps)
            k = log_prob / math.log(p_no)
        i += 1
        out.iterations = i
    return out


# ---- the whole of detect()
@dataclass
class Floor:
    detected: bool
    reason: int
    n_clipped: int
    n_filtered: int
    n_inliers: int
    ransac_iterations: int
    coeffs: np.ndarray            # float32[4] (zeros when not detected)
    filtered: np.ndarray          # indices into the input of the RANSAC input
    inliers: np.ndarray           # indices into the input of the model's inliers
    ransac: Ransac | None = None
    clip: np.ndarray | None = None
    normals: Normals | None = None


def detect(p: FloorParams, cloud) -> Floor:
    clip = clip_flags(p, cloud)
    ci = np.flatnonzero(clip)
    f32 = xyz32(cloud)
    nrm = None
    fi = ci
    if p.use_normal_filtering:
        nrm = normals(p, f32[ci])
        fi = ci[nrm.keep]
    none = np.zeros(0, np.int64)
    res = Floor(False, TOO_FEW_POINTS, len(ci), len(fi), 0, 0, np.zeros(4, np.float32), fi, none, None, clip, nrm)
    if len(fi) == 0 or len(fi) < p.floor_pts_thresh:
        return res
    pts = f32[fi].astype(np.float64)
    rs = ransac(p, pts)
    res.ransac, res.ransac_iterations = rs, rs.iterations
    co = rs.plane.astype(np.float32)
    inl = np.zeros(len(fi), bool) if rs.best_i < 0 else distances(co.astype(np.float64), pts) < p.ransac_distance_threshold
    res.inliers, res.n_inliers = fi[inl], int(inl.sum())
    if res.n_inliers < p.floor_pts_thresh or rs.best_i < 0:
        res.reason = TOO_FEW_INLIERS
        return res
    rx, rz = direction(p)
    dot = float(co[0]) * float(rx) + float(co[2]) * float(rz)
    if abs(dot) < math.cos(p.floor_normal_thresh * math.pi / 180.0):
        res.reason = NOT_VERTICAL
        return res
    if co[2] < 0:
        co = -co
    res.detected, res.reason, res.coeffs = True, DETECTED, co
    return res
