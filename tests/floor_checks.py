"""Shared checks of the floor detection (hgs_detect_floor and its two stage hooks) against the restatement of tests/floor_reference.py:
tests/test_floor_simt_host.py runs them on the host emulation of the kernels, tests/test_floor_gpu.py on the MI355X.  `make(pnh, **constants)`
builds a hdl_graph_slam_amd.FloorDetector on the library under test."""
from __future__ import annotations

import functools
import math

import numpy as np

import floor_reference as FR
from hdl_graph_slam_amd import synth

INPUTS = {"vlp16": ("VLP-16", 1, 0.3), "hdl32": ("HDL-32E", 4, 0.5)}


@functools.lru_cache(maxsize=None)
def scan(kind: str) -> np.ndarray:
    sensor, seed, ds = INPUTS[kind]
    cloud = synth.make_pair(sensor, seed, downsample=ds)[0]
    cloud.setflags(write=False)
    return cloud


def records(xyz, intensity=None) -> np.ndarray:
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros(len(xyz), synth.POINT_XYZI_DTYPE)
    out["x"], out["y"], out["z"], out["w"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0
    out["intensity"] = np.arange(len(xyz), dtype=np.float32) if intensity is None else intensity
    return out


def ref_params(pnh=None, **constants) -> FR.FloorParams:
    p = FR.FloorParams()
    for k, v in {**(pnh or {}), **constants}.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _reference_cached(kind: str, key):
    return FR.detect(ref_params(dict(key)), scan(kind))


def reference(kind: str, pnh=None) -> FR.Floor:
    """The reference's result on one of the named inputs, computed once per parameter set."""
    return _reference_cached(kind, tuple(sorted((pnh or {}).items())))


# ---- clip
def check_clip_tilt0(make):
    h, clip = 2.0, 1.0
    lo, hi = np.float32(-(h + clip)), np.float32(-(h - clip))
    inf = np.float32(np.inf)
    edge = [[1, 2, lo], [1, 2, hi], [1, 2, np.nextafter(lo, -inf)], [1, 2, np.nextafter(lo, inf)], [1, 2, np.nextafter(hi, -inf)], [1, 2, np.nextafter(hi, inf)]]
    want_edge = [True, False, False, True, True, False]
    bad = []
    for v in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            row = [1.0, 2.0, -2.0]
            row[axis] = v
            bad.append(row)
    cloud = np.concatenate([scan("vlp16"), records(edge), records(bad)])
    pnh = {"use_normal_filtering": False}
    d = make(pnh)
    dc = d.engine.upload(cloud)
    k1, k2, _ = d.debug_filter(dc)
    want = FR.clip_flags(ref_params(pnh), cloud)
    n = len(scan("vlp16"))
    assert want[n:n + 6].tolist() == want_edge            # the reference itself: PCL's >= 0 rule on both planes
    assert not want[n + 6:].any()
    assert np.array_equal(k1, want)
    assert np.array_equal(k2, want)                       # without the normal filter the second flag is the first
    assert 100 < want.sum() < n
    dc.close()
    d.close()


def check_clip_tilted(make):
    pnh = {"tilt_deg": 3.0, "use_normal_filtering": False}
    cloud = scan("vlp16")
    d = make(pnh)
    dc = d.engine.upload(cloud)
    k1, _, _ = d.debug_filter(dc)
    p = ref_params(pnh)
    want = FR.clip_flags(p, cloud)
    z = FR.clip_z64(p, cloud)
    band = (np.abs(z + (p.sensor_height + p.height_clip_range)) <= 1e-5) | (np.abs(z + (p.sensor_height - p.height_clip_range)) <= 1e-5)
    print(f"tilted clip: {band.sum()} of {len(cloud)} points in the band, {(k1 != want).sum()} flags differ")
    assert band.sum() <= 0.01 * len(cloud)
    assert np.array_equal(k1[~band], want[~band])
    assert not np.array_equal(want, FR.clip_flags(ref_params({"use_normal_filtering": False}), cloud))    # the tilt matters on this input
    dc.close()
    d.close()


# ---- normal filter
def check_normals(make, kind):
    cloud = scan(kind)
    d = make({})
    dc = d.engine.upload(cloud)
    k1, k2, nrm = d.debug_filter(dc)
    ref = reference(kind)
    assert np.array_equal(k1, ref.clip)
    ci = np.flatnonzero(ref.clip)
    rn = ref.normals
    out = rn.tie | rn.degenerate | rn.in_band
    print(f"normals {kind}: {len(ci)} clipped, ties {rn.tie.sum()}, in band {rn.in_band.sum()}, near-degenerate {rn.degenerate.sum()}, left out {out.mean():.4%}")
    assert out.sum() <= 0.01 * len(ci)
    assert np.array_equal(k2[ci][~out], rn.keep[~out])
    assert not k2[~ref.clip].any() and np.isnan(nrm[~ref.clip]).all()
    got = nrm[ci][~out]
    sign = np.sign((got * rn.normals[~out]).sum(1))[:, None]
    dev = np.abs(got * sign - rn.normals[~out]).max()
    print(f"normals {kind}: worst component deviation {dev:.3e}")
    assert dev <= 1e-9
    assert np.abs(np.linalg.norm(nrm[ci], axis=1) - 1.0).max() <= 1e-12
    dc.close()
    d.close()


# ---- RANSAC counts
def _check_counts(d, pts, p, n_hyp=200):
    dc = d.engine.upload(pts)
    counts, planes = d.debug_ransac_counts(dc, 0, n_hyp)
    dc.close()
    p64 = FR.xyz64(pts)
    left_out = 0
    for i in range(n_hyp):
        c, pl, near = FR.hypothesis(p, p64, i)
        assert np.abs(planes[i] - pl).max() <= 1e-12, (len(pts), i, planes[i], pl)
        if near:
            left_out += 1
            continue
        assert counts[i] == c, (len(pts), i, counts[i], c)
    assert left_out <= 0.01 * n_hyp, (len(pts), left_out)
    return counts


def check_ransac_counts(make):
    pnh = {"use_normal_filtering": False}
    p = ref_params(pnh, seed=7)
    d = make(pnh, seed=7)
    cloud = scan("vlp16")
    big = cloud[FR.clip_flags(p, cloud)]
    assert 2000 < len(big) < 4000
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        c = _check_counts(d, big[:n], p)
        assert (c == 0).all() if n < 3 else c.max() >= 3
    c = _check_counts(d, big, p)
    assert c.max() > 0.5 * len(big)                       # some hypothesis lies in the floor
    # degenerate triples score 0: three collinear points (every triple is that one), and a cloud of identical points
    line = records([[0, 0, -2], [1, 1, -2], [2, 2, -2]])
    same = records(np.tile([[1.5, -2.5, -2.0]], (100, 1)))
    for pts in (line, same):
        dc = d.engine.upload(pts)
        counts, planes = d.debug_ransac_counts(dc, 0, 50)
        assert (counts == 0).all() and (planes == 0).all()
        dc.close()
    # i0: hypotheses 150..199 on their own are the tail of 0..199
    dc = d.engine.upload(big)
    all_c, all_p = d.debug_ransac_counts(dc, 0, 200)
    tail_c, tail_p = d.debug_ransac_counts(dc, 150, 50)
    assert np.array_equal(all_c[150:], tail_c) and np.array_equal(all_p[150:], tail_p)
    dc.close()
    d.close()


# ---- the sequential rule, chunking
@functools.lru_cache(maxsize=None)
def patch_cloud() -> np.ndarray:
    """30 % floor patch (z = -2 +- 2 cm) and 70 % clutter, uniform over the clip band outside 15 cm of the patch (clutter inside the threshold would
    count as floor): w = 0.30, and the rule needs log(0.01) / log(1 - 0.3^3) = 168 hypotheses once it has found the patch."""
    rng = np.random.default_rng(5)
    n, nf = 3000, 900
    floor = np.stack([rng.uniform(-10, 10, nf), rng.uniform(-10, 10, nf), -2.0 + rng.uniform(-0.02, 0.02, nf)], 1)
    clutter = np.stack([rng.uniform(-10, 10, n - nf), rng.uniform(-10, 10, n - nf), rng.uniform(0.15, 0.99, n - nf) * rng.choice([-1.0, 1.0], n - nf) - 2.0], 1)
    pts = np.concatenate([floor, clutter])[rng.permutation(n)]
    out = records(pts)
    out.setflags(write=False)
    return out


def _record(d):
    r = d.last
    return bytes(r)


def check_sequential_rule(make):
    pnh = {"use_normal_filtering": False}
    cloud = patch_cloud()
    ref = FR.detect(ref_params(pnh), cloud)
    assert ref.detected and 120 <= ref.ransac_iterations <= 220 and not ref.ransac.near
    d = make(pnh)
    dc = d.engine.upload(cloud)
    blobs = []
    for chunk in (64, 1, 7, 1000, 64):
        d.engine.set_option("floor_chunk", chunk)
        co = d.detect(dc)
        r = d.last
        assert (r.detected, r.reason, r.n_clipped, r.n_filtered, r.n_inliers, r.ransac_iterations) == (
            1, FR.DETECTED, ref.n_clipped, ref.n_filtered, ref.n_inliers, ref.ransac_iterations), chunk
        assert np.array_equal(co, ref.coeffs), (chunk, co, ref.coeffs)
        blobs.append(_record(d))
    assert len(set(blobs)) == 1                           # byte-identical for every chunk size and across two runs (64 twice)
    # the chosen hypothesis: its plane through the counts hook, rounded to float, is the model (up to the upward flip)
    _, planes = d.debug_ransac_counts(dc, ref.ransac.best_i, 1)
    model = planes[0].astype(np.float32)
    assert np.array_equal(co, model if model[2] >= 0 else -model)
    for max_it in (0, 1, 5):
        dm = make(pnh, ransac_max_iterations=max_it)
        dcm = dm.engine.upload(cloud)
        rm = FR.detect(ref_params(pnh, ransac_max_iterations=max_it), cloud)
        assert rm.ransac_iterations == max_it
        for chunk in (1, 64):
            dm.engine.set_option("floor_chunk", chunk)
            co = dm.detect(dcm)
            r = dm.last
            assert (r.detected, r.reason, r.n_inliers, r.ransac_iterations) == (int(rm.detected), rm.reason, rm.n_inliers, rm.ransac_iterations), (max_it, chunk)
            assert (co is None) == (not rm.detected) and (co is None or np.array_equal(co, rm.coeffs))
        dcm.close()
        dm.close()
    dc.close()
    d.close()


# ---- end to end
def ulp_close(a, b) -> bool:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def compare(d, got, ref: FR.Floor, cloud):
    r = d.last
    assert (r.detected, r.reason, r.n_clipped, r.n_filtered, r.n_inliers) == (int(ref.detected), ref.reason, ref.n_clipped, ref.n_filtered, ref.n_inliers)
    assert r.ransac_iterations == ref.ransac_iterations
    fp = d.filtered_points()
    assert fp is not None and fp[["x", "y", "z", "intensity"]].tobytes() == cloud[ref.filtered][["x", "y", "z", "intensity"]].tobytes()
    if not ref.detected:
        assert got is None and d.floor_points() is None and not np.any(np.array(r.coeffs))
        return
    assert ulp_close(got, ref.coeffs), (got, ref.coeffs)
    assert got[2] >= 0
    ip = d.floor_points()
    assert ip[["x", "y", "z", "intensity"]].tobytes() == cloud[ref.inliers][["x", "y", "z", "intensity"]].tobytes()


def check_end_to_end(make, kind):
    cloud = scan(kind)
    for pnh in ({}, {"use_normal_filtering": False}):
        ref = reference(kind, pnh)
        assert ref.detected and ref.n_inliers > 1000
        d = make(pnh)
        compare(d, d.detect(cloud), ref, cloud)
        d.close()


def check_cloud_end_to_end(make, cloud, pnh=None, **constants):
    ref = FR.detect(ref_params(pnh, **constants), cloud)
    d = make(pnh, **constants)
    compare(d, d.detect(cloud), ref, cloud)
    d.close()
    return ref


def check_rejections(make):
    cloud = scan("vlp16")
    base = reference("vlp16")
    assert base.n_inliers < base.n_filtered
    for thresh, reason in ((base.n_filtered + 1, FR.TOO_FEW_POINTS), (base.n_inliers + 1, FR.TOO_FEW_INLIERS), (base.n_inliers, FR.DETECTED)):
        ref = check_cloud_end_to_end(make, cloud, {"floor_pts_thresh": thresh})
        assert ref.reason == reason
    rng = np.random.default_rng(2)
    wall = records(np.stack([np.full(2000, 5.0) + rng.uniform(-0.01, 0.01, 2000), rng.uniform(-5, 5, 2000), rng.uniform(-2.9, -1.1, 2000)], 1))
    ref = check_cloud_end_to_end(make, wall, {"use_normal_filtering": False, "floor_normal_thresh": 10.0})
    assert ref.reason == FR.NOT_VERTICAL and ref.n_inliers >= 512
    ref = check_cloud_end_to_end(make, wall, {})          # with the normal filter nothing of a wall is left
    assert ref.reason == FR.TOO_FEW_POINTS and ref.n_filtered < 512


def check_upside_down(make):
    """The scene turned about x by 180 degrees: the floor is above the sensor (sensor_height -1.2 puts the clip around it); whichever way the
    triple's normal points, the result's normal points up."""
    cloud = scan("vlp16").copy()
    cloud["y"], cloud["z"] = -cloud["y"], -cloud["z"]
    signs = set()
    for seed in range(4):
        pnh = {"sensor_height": -1.2}
        ref = check_cloud_end_to_end(make, cloud, pnh, seed=seed)
        assert ref.detected and ref.coeffs[2] > 0.99 and ref.coeffs[3] < -1.0
        signs.add(bool(ref.ransac.plane[2] < 0))
    assert signs == {True, False}                         # the flip of :164-166 ran for some seed and not for another


def check_prefilter_output_goes_in_resident(make, raw):
    d = make({})
    dc = d.engine.prefilter(raw)
    got = d.detect(dc)
    cloud = dc.download()
    ref = FR.detect(ref_params({}), cloud)
    assert ref.n_clipped > 500
    compare(d, got, ref, cloud)
    dc.close()
    d.close()


# ---- errors
def check_errors(make, HgsError):
    import pytest
    cloud = scan("vlp16")
    bad = [({"floor_pts_thresh": -1}, {}), ({"height_clip_range": -0.5}, {}), ({"floor_normal_thresh": -1.0}, {}), ({"normal_filter_thresh": -1.0}, {}),
           ({}, {"ransac_distance_threshold": -0.1}), ({}, {"ransac_max_iterations": -1}), ({}, {"normal_k": 2}), ({}, {"normal_k": 65}),
           ({}, {"ransac_probability": 0.0}), ({}, {"ransac_probability": 1.0}), ({"tilt_deg": float("nan")}, {})]
    for pnh, constants in bad:
        d = make(pnh, **constants)
        with pytest.raises(HgsError, match="invalid argument"):
            d.detect(cloud)
        dc = d.engine.upload(cloud)
        with pytest.raises(HgsError, match="invalid argument"):
            d.debug_filter(dc)
        with pytest.raises(HgsError, match="invalid argument"):
            d.debug_ransac_counts(dc, 0, 4)
        dc.close()
        d.close()
    for constants in ({"normal_k": 3}, {"normal_k": 64}):     # the ends of the allowed range run
        check_cloud_end_to_end(make, cloud, {}, **constants)
    a, b = make({}), make({})
    foreign = b.engine.upload(cloud)
    with pytest.raises(HgsError, match="invalid argument"):
        a.detect(foreign)
    assert b.detect(foreign) is not None
    foreign.close()
    b.close()
    # an empty cloud, nothing inside the clip, fewer clipped points than normal_k: not detected, TOO_FEW_POINTS
    empty = np.zeros(0, synth.POINT_XYZI_DTYPE)
    above = records([[1, 1, 5.0], [2, 1, 4.0], [3, 3, 0.0]])
    rng = np.random.default_rng(3)
    few = np.concatenate([above, records(np.stack([rng.uniform(-3, 3, 5), rng.uniform(-3, 3, 5), rng.uniform(-2.5, -1.5, 5)], 1))])
    for pts, n_clipped in ((empty, 0), (above, 0), (few, 5)):
        for nf in (True, False):
            pnh = {"use_normal_filtering": nf}
            d = make(pnh)
            co = d.detect(pts)
            ref = FR.detect(ref_params(pnh), pts)
            r = d.last
            assert co is None and (r.detected, r.reason, r.n_clipped, r.n_inliers, r.ransac_iterations) == (0, FR.TOO_FEW_POINTS, n_clipped, 0, 0)
            assert ref.n_clipped == n_clipped and r.n_filtered == ref.n_filtered
            fp = d.filtered_points()
            assert fp is not None and len(fp) == ref.n_filtered
            d.close()
    # ... and with a threshold of 0 the five points go through RANSAC like any cloud
    check_cloud_end_to_end(make, few, {"floor_pts_thresh": 0, "use_normal_filtering": False})
    a.close()


# ---- the Python mirror
def check_python_mirror(make):
    from hdl_graph_slam_amd.floor_detection import floor_params_from_rosparams
    p = floor_params_from_rosparams({})
    assert (p.tilt_deg, p.sensor_height, p.height_clip_range, p.floor_pts_thresh, p.floor_normal_thresh, bool(p.use_normal_filtering), p.normal_filter_thresh) == (
        0.0, 2.0, 1.0, 512, 10.0, True, 20.0)             # apps/floor_detection_nodelet.cpp:57-63
    assert (p.normal_k, p.ransac_distance_threshold, p.ransac_max_iterations, p.ransac_probability, p.seed) == (10, 0.1, 1000, 0.99, 0)
    q = floor_params_from_rosparams({"tilt_deg": 1.5, "sensor_height": 1.7, "height_clip_range": 0.5, "floor_pts_thresh": 100, "floor_normal_thresh": 5.0,
                                     "use_normal_filtering": False, "normal_filter_thresh": 15.0, "points_topic": "/velodyne_points"}, seed=9)
    assert (q.tilt_deg, q.sensor_height, q.height_clip_range, q.floor_pts_thresh, q.floor_normal_thresh, q.use_normal_filtering, q.normal_filter_thresh, q.seed) == (
        1.5, 1.7, 0.5, 100, 5.0, 0, 15.0, 9)
    d = make({"floor_pts_thresh": 100000})
    assert d.detect(scan("vlp16")) is None and d.reason == "TOO_FEW_POINTS" and d.floor_points() is None and d.filtered_points() is not None
    d.params.floor_pts_thresh = 512
    co = d.detect(scan("vlp16"))
    assert co is not None and co.dtype == np.float32 and co.shape == (4,) and d.reason == "DETECTED"
    assert abs(math.sqrt(float(co[0]) ** 2 + float(co[1]) ** 2 + float(co[2]) ** 2) - 1.0) < 1e-6
    d.close()
