"""Host-only checks of tests/floor_reference.py itself (no library under test): the generator, the plane and count arithmetic, the sequential rule and
the acceptance tests on inputs whose answer is known."""
import math

import numpy as np

import floor_checks as FC
import floor_reference as FR


def test_generator_gives_three_distinct_indices_and_depends_on_every_argument():
    for n in (3, 4, 5, 17, 1000, 2 ** 31 - 1):
        seen = set()
        for i in range(300):
            t = FR.sample3(11, i, n)
            assert len(set(t)) == 3 and all(0 <= v < n for v in t)
            seen.add(t)
        assert n < 6 or len(seen) > 250
    assert FR.sample3(1, 5, 1000) != FR.sample3(2, 5, 1000) != FR.sample3(2, 6, 1000)
    assert FR.sample3(1, 5, 1000) == FR.sample3(1, 5, 1000)
    # every ordered triple of a three-point cloud's indices is a permutation, and every index turns up in every position
    firsts = {FR.sample3(0, i, 5)[k] for i in range(200) for k in range(3)}
    assert firsts == {0, 1, 2, 3, 4}
    assert FR.mix64(0) == 0 and FR.mix64(1) == 0x5692161D100B05E5          # splitmix64's finaliser


def test_plane_and_counts_on_a_known_plane():
    pts = np.array([[0, 0, -2.0], [1, 0, -2.0], [0, 1, -2.0], [5, 5, -2.05], [5, 5, -1.9], [5, 5, -2.1]])
    pl = FR.plane3(pts, 0, 1, 2)
    assert np.allclose(pl, [0, 0, 1, 2.0], atol=1e-15)
    assert FR.plane3(pts, 0, 2, 1)[2] == -1.0                                # the triple's order decides the sign
    d = FR.distances(pl, pts)
    assert ((d < 0.1) == [True, True, True, True, False, False]).all()       # strict: |-2.1 + 2| = 0.1 is rounding away from 0.1 either way
    assert FR.plane3(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2.0]]), 0, 1, 2) is None


def test_sequential_rule_stops_where_pcl_stops():
    cloud = FC.patch_cloud()
    p = FC.ref_params({"use_normal_filtering": False})
    pts = FR.xyz64(cloud)
    rs = FR.ransac(p, pts)
    w = rs.best / len(pts)
    k = math.log(1 - 0.99) / math.log(1 - w ** 3)
    assert rs.iterations == min(math.ceil(k), 1000) and 0.29 < w < 0.31
    assert rs.best == max(FR.hypothesis(p, pts, i)[0] for i in range(rs.iterations))
    assert rs.best_i == min(i for i in range(rs.iterations) if FR.hypothesis(p, pts, i)[0] == rs.best)      # strict >: the first best stays
    for m in (0, 1, 5):
        assert FR.ransac(FC.ref_params(ransac_max_iterations=m), pts).iterations == m
    # a degenerate first triple: count 0 does not beat best = 0, k stays 1, the search ends after one iteration without a model
    same = np.tile([[1.0, 2.0, -2.0]], (600, 1))
    rs = FR.ransac(p, same)
    assert (rs.iterations, rs.best, rs.best_i) == (1, 0, -1)
    out = FR.detect(p, FC.records(same))
    assert (out.detected, out.reason, out.n_filtered, out.n_inliers) == (False, FR.TOO_FEW_INLIERS, 600, 0)


def test_detect_on_the_scans():
    for kind, height in (("vlp16", 1.2), ("hdl32", 1.5)):
        ref = FC.reference(kind)
        assert ref.detected and abs(ref.coeffs[3] - height) < 0.05 and ref.coeffs[2] > 0.999
        assert ref.n_clipped >= ref.n_filtered >= ref.n_inliers > 1000
        assert np.all(np.diff(ref.filtered) > 0) and np.all(np.diff(ref.inliers) > 0) and set(ref.inliers) <= set(ref.filtered)
        rn = ref.normals
        assert (rn.tie | rn.degenerate | rn.in_band).mean() <= 0.01
        assert np.abs(np.linalg.norm(rn.normals, axis=1) - 1).max() < 1e-12


def test_clip_follows_pcls_rule_and_drops_non_finite_points():
    p = FR.FloorParams()
    z = np.float32([-3.0, np.nextafter(np.float32(-3), np.float32(-4)), -1.0, np.nextafter(np.float32(-1), np.float32(-2)), -2.0, 0.0])
    pts = np.stack([np.ones(6, np.float32), np.ones(6, np.float32), z], 1)
    assert FR.clip_flags(p, pts).tolist() == [True, False, False, True, True, False]
    bad = np.float32([[np.nan, 0, -2], [0, np.inf, -2], [0, 0, -np.inf], [np.inf, 0, -2]])
    assert not FR.clip_flags(p, bad).any()
    rx, rz = FR.direction(FR.FloorParams(tilt_deg=3.0))
    assert abs(float(rx) + math.sin(math.radians(3))) < 1e-7 and abs(float(rz) - math.cos(math.radians(3))) < 1e-7
