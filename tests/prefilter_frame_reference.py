"""The yardstick of the prefilter's base_link transform (hgs_prefilter_framed, pf_transform_point of hgs_math.h): pcl::transformPointCloud with a float
matrix as PCL >= 1.10 computes it (pcl/common/impl/transforms.hpp, Transformer<float>::se3), restated in numpy — per row r

    x * m(r, 0) + (y * m(r, 1) + (z * m(r, 2) + m(r, 3)))

with every product and every sum rounded to np.float32 (numpy's float32 array arithmetic rounds once per operation and fuses nothing).  A point with a
non-finite coordinate passes through untouched, as PCL passes it through in a cloud that is not dense; every other field of a record is copied.
tests/test_prefilter_frame_host.py holds this restatement to the mock pcl::transformPointCloud of tests/mock_pcl compiled with -ffp-contract=off."""
from __future__ import annotations

import numpy as np


def matrix32(T) -> np.ndarray:
    """The 4x4 as the float matrix the transform is computed with."""
    m = np.asarray(T, dtype=np.float32)
    assert m.shape == (4, 4)
    return m


def transform_xyz(xyz: np.ndarray, T) -> np.ndarray:
    """[n, 3] float32 -> [n, 3] float32."""
    m = matrix32(T)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = xyz.copy()
    finite = np.isfinite(xyz).all(axis=1)
    with np.errstate(all="ignore"):
        for r in range(3):
            v = x * m[r, 0] + (y * m[r, 1] + (z * m[r, 2] + m[r, 3]))
            assert v.dtype == np.float32
            out[finite, r] = v[finite]
    return out


def transform(cloud: np.ndarray, T) -> np.ndarray:
    """PointXYZI records -> PointXYZI records (x, y, z transformed; w, intensity and padding copied)."""
    out = np.array(cloud, copy=True)
    new = transform_xyz(np.stack([cloud["x"], cloud["y"], cloud["z"]], axis=1), T)
    out["x"], out["y"], out["z"] = new[:, 0], new[:, 1], new[:, 2]
    return out


def rigid(axis, angle: float, translation) -> np.ndarray:
    """A rigid 4x4 (float64): Rodrigues' rotation about `axis` by `angle`, then `translation`."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = translation
    return T
