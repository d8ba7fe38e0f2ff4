"""TEST-SIDE RESTATEMENT of the prefilter's two outlier filters (apps/prefiltering_nodelet.cpp:73-93, :151-163) by brute force in plain numpy,
and of pcl::ApproximateVoxelGrid as a sequential loop.  oracle/prefilter.hpp — which the device is compared with bit for bit — is held to this;
nothing here goes through the oracle's library, a search tree or the device.

UPSTREAM-KNOWLEDGE (PCL is not vendored with the reference; written from PCL's documented behaviour, functions cited by name only):

  pcl::RadiusOutlierRemoval::applyFilterIndices: a radius search around every point, which finds the point itself; the point is kept iff the
    search returns MORE than min_neighbors points.  FLANN's radius search is strict: d2 < r * r, with r * r computed in double and handed over
    as a float.
  pcl::StatisticalOutlierRemoval::applyFilterIndices: a (mean_k + 1)-nearest search around every point; the first result (the point itself, or a
    coincident point: distance 0 either way) is skipped, the other distances — sqrt of the float d2, taken in double — are summed in ascending
    order and divided by mean_k.  Over these d_i: sum and sum of squares in double, mean = sum / n, variance = (sq - sum * sum / n) / (n - 1),
    threshold = mean + stddev_mul * sqrt(variance); a point is kept iff d_i <= threshold.

Stated deviations from PCL, shared by the oracle and the device (prefilter):
  * non-finite points take no part: not in the search, not in the statistics (n is the number of finite points), not in the output.  PCL keeps
    the non-finite points of a non-dense cloud in the output as inliers while leaving them out of the statistics;
  * a cloud of fewer than mean_k + 1 finite points: the distances that were found are summed and still divided by mean_k; a single point has d = 0;
  * ties in the k-th distance go to the lowest original index (FLANN's order among equidistant points is unspecified).

Arithmetic.  The float squared distance is the one of the search both sides use — hgs_math.h dist2f on the device, oracle/kdtree.hpp dist2f in
the oracle's tree: dx, dy, dz float differences (query minus point), d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).  `fmaf32` below is that fused
operation EXACTLY: the product of two floats is exact in double, the double sum is corrected to round-to-odd with the error term of the
two-sum, and a round-to-odd double (53 >= 24 + 2 bits) rounds to the same float as the infinitely precise result — no double rounding."""
from __future__ import annotations

import numpy as np


def fmaf32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf(a, b, c) for finite float32 arrays, correctly rounded."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                       # exact: 24 x 24 bits
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)   # two-sum: p + c = s + err exactly
    bits = s.view(np.int64)
    inexact_even = (err != 0) & ((bits & 1) == 0)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(inexact_even, np.nextafter(s, toward), s)   # round to odd
    return s.astype(np.float32)


def xyz_intensity(cloud) -> np.ndarray:
    """[n, 4] float32 {x, y, z, intensity} of PointXYZI records or of an [n, >= 4] array that already is in this form."""
    if getattr(cloud, "dtype", None) is not None and cloud.dtype.fields is not None:
        return np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :4])


def finite_rows(pts4: np.ndarray) -> np.ndarray:
    return np.isfinite(pts4[:, :3]).all(axis=1)


def dist2_matrix(xyz: np.ndarray) -> np.ndarray:
    """d2[i, j] = dist2f(point i as the query, point j), float32."""
    xyz = np.asarray(xyz, np.float32)
    d = xyz[:, None, :] - xyz[None, :, :]       # float subtraction
    s = (d[..., 0].astype(np.float64) * d[..., 0].astype(np.float64)).astype(np.float32)   # dx * dx: one rounding of an exact product
    s = fmaf32(d[..., 1], d[..., 1], s)
    return fmaf32(d[..., 2], d[..., 2], s)


def radius_outlier_keep(pts4: np.ndarray, radius: float, min_neighbors: int) -> np.ndarray:
    """Keep flags, one per input point (non-finite points: False)."""
    pts4 = xyz_intensity(pts4)
    ok = finite_rows(pts4)
    keep = np.zeros(len(pts4), bool)
    if ok.any():
        r2 = np.float32(float(radius) * float(radius))
        keep[ok] = (dist2_matrix(pts4[ok, :3]) < r2).sum(axis=1) > int(min_neighbors)
    return keep


def radius_outlier_removal(pts4, radius: float, min_neighbors: int) -> np.ndarray:
    pts4 = xyz_intensity(pts4)
    return pts4[radius_outlier_keep(pts4, radius, min_neighbors)]


def _serial_sum(values, reverse: bool) -> tuple[float, float]:
    s = q = 0.0
    for v in (reversed(values) if reverse else values):
        v = float(v)
        s += v
        q += v * v
    return s, q


def statistical_outlier_details(pts4, mean_k: int, stddev_mul: float, reverse_sums: bool = False):
    """(keep flags per input point, d_i of the finite points in input order, threshold).  reverse_sums takes the sum and the sum of squares from
    the last point to the first: the flags of a well-conditioned case do not depend on the order."""
    pts4 = xyz_intensity(pts4)
    ok = finite_rows(pts4)
    n = int(ok.sum())
    keep = np.zeros(len(pts4), bool)
    if n == 0:
        return keep, np.zeros(0), 0.0
    d2 = dist2_matrix(pts4[ok, :3])
    order = np.argsort(d2, axis=1, kind="stable")    # ascending d2, ties to the lowest index
    found = min(int(mean_k) + 1, n)
    near = np.take_along_axis(d2, order[:, :found], axis=1)
    total = np.zeros(n)
    for j in range(1, found):                        # ascending, the first dropped
        total = total + np.sqrt(near[:, j].astype(np.float64))
    d = total / float(mean_k) if found > 1 else np.zeros(n)
    s, q = _serial_sum(list(d), reverse_sums)
    mean = s / n
    var = (q - s * s / n) / (n - 1.0) if n > 1 else 0.0
    thr = mean + float(stddev_mul) * float(np.sqrt(var))
    keep[ok] = d <= thr
    return keep, d, thr


def statistical_outlier_removal(pts4, mean_k: int, stddev_mul: float) -> np.ndarray:
    pts4 = xyz_intensity(pts4)
    return pts4[statistical_outlier_details(pts4, mean_k, stddev_mul)[0]]


def threshold_band(d: np.ndarray, thr: float, rel: float = 1e-12) -> np.ndarray:
    """The statistical filter's points whose flag the summation order may decide: within rel * thr of a positive threshold.  (A threshold of exactly 0
    means every d_i is 0 — the sums are then exact in any order, nothing is in doubt.)"""
    if not thr > 0:
        return np.zeros(len(d), bool)
    return np.abs(d - thr) <= rel * thr


def approx_voxelgrid(cloud, leaf):
    """pcl::ApproximateVoxelGrid as PCL runs it — a plain sequential loop over the points with the 512-entry history table —
    independent of oracle/prefilter.hpp and of the device's sort-based form."""
    inv = np.float32(1.0) / np.float32(leaf)
    hist = {}
    out = []

    def flush(e):
        out.append((e[4] / np.float32(e[3])).astype(np.float32))

    for r in cloud:
        p = np.array([r["x"], r["y"], r["z"], r["intensity"]], np.float32)
        if not np.isfinite(p[:3]).all():
            continue
        ix, iy, iz = (int(np.floor(np.float32(p[k] * inv))) for k in range(3))
        h = (ix * 7171 + iy * 3079 + iz * 4231) & 511
        e = hist.get(h)
        if e is not None and e[3] and (e[0], e[1], e[2]) != (ix, iy, iz):
            flush(e)
            e = None
        if e is None:
            e = [ix, iy, iz, 0, np.zeros(4, np.float32)]
            hist[h] = e
        e[3] += 1
        e[4] = (e[4] + p).astype(np.float32)
    for h in sorted(hist):
        if hist[h][3]:
            flush(hist[h])
    return np.array(out, np.float32).reshape(-1, 4)
