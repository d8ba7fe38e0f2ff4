"""Shared checks of the prefilter (hgs_prefilter: kernels k_pf_* of hgs_kernels.hip, host sequence prefilter_impl of hgs_engine.hip) at the inputs where
these kernels can go wrong — every instantiation of the k-NN distance kernel and both sides of its bounds, clouds smaller than k + 1, one wave plus or
minus one, coincident points, non-finite points in front of the outlier filters, one voxel several blocks long, exact block multiples, the distance
filter's strict thresholds, the voxel index overflow, parameter validation.  tests/test_prefilter.py runs them on the MI355X (-m gpu),
tests/test_simt_kernels_host.py on the host emulation of the same kernels.  `make_engine(params)` builds a RegistrationHIP on the library under test.

Every device result is compared with the oracle (oracle/prefilter.hpp) point for point, in order, bit for bit; the oracle's two outlier filters are held
to tests/prefilter_reference.py on the same outlier_cases() by tests/test_prefilter.py.  Clouds are synthetic and of a few hundred points (3000 once)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import oracle as O
import prefilter_reference as PR
from hdl_graph_slam_amd import synth

NONE, VOXELGRID, APPROX = 0, 1, 2       # HGS_DOWNSAMPLE_*
STATISTICAL, RADIUS = 1, 2              # HGS_OUTLIER_*


# ---- inputs (computed once, read-only)
def _frozen(cloud: np.ndarray) -> np.ndarray:
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def mixture(n: int = 600, seed: int = 0) -> np.ndarray:
    """A dense core with stragglers: normal(0, 3), every fifth point from normal(0, 30)."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0, 3, (n, 3)).astype(np.float32)
    xyz[::5] = rng.normal(0, 30, (len(xyz[::5]), 3)).astype(np.float32)
    return _frozen(synth.to_xyzi(xyz, rng.uniform(0, 255, n)))


@functools.lru_cache(maxsize=None)
def nonfinite_mixture() -> np.ndarray:
    """The mixture with a third of its points non-finite: NaN in x and inf in z, alternately."""
    cloud = mixture(600, 1).copy()
    cloud["x"][0::6] = np.nan
    cloud["z"][3::6] = np.inf
    return _frozen(cloud)


@functools.lru_cache(maxsize=None)
def negative_box() -> np.ndarray:
    """A flat box around the origin: negative coordinates, negative voxel indices."""
    rng = np.random.default_rng(2)
    return _frozen(synth.to_xyzi((rng.uniform(-1, 1, (500, 3)) * [40, 40, 3]).astype(np.float32), rng.uniform(0, 255, 500)))


@functools.lru_cache(maxsize=None)
def duplicates() -> np.ndarray:
    return _frozen(np.concatenate([mixture()[:100]] * 3))


def _stat(mean_k=20, stddev=1.0, downsample=NONE, leaf=0.5):
    return dict(use_distance_filter=0, downsample_method=downsample, downsample_resolution=leaf, outlier_removal_method=STATISTICAL,
                statistical_mean_k=mean_k, statistical_stddev=stddev)


def _radius(radius, min_neighbors, downsample=NONE, leaf=0.5, use_filter=0):
    return dict(use_distance_filter=use_filter, downsample_method=downsample, downsample_resolution=leaf, outlier_removal_method=RADIUS,
                radius_radius=radius, radius_min_neighbors=min_neighbors)


STAT_MEAN_K = (1, 15, 16, 31, 32, 40, 62)     # both sides of KMAX 16 | 32 | 64 (launch_pf_mean_knn_dist), the bounds 1 and 62, one well inside the last
STAT_STDDEV = (0.0, 1.0, 2.5)
STAT_SIZES = (1, 2, 5, 20, 21, 22, 63, 64, 65, 257)   # at mean_k = 20: fewer than k + 1 points, exactly k + 1, one wave +- 1, a second block
RADIUS_MIN_NEIGHBORS = (0, 2, 50)
RADIUS_SIZES = (1, 2, 65)
DOWNSAMPLE_NAMES = {NONE: "none", VOXELGRID: "voxelgrid", APPROX: "approx"}


@functools.lru_cache(maxsize=None)
def outlier_cases() -> dict:
    """name -> (cloud, prefilter parameters by field name): what the device is compared with the oracle on, and the oracle with the numpy reference."""
    cases = {}
    for k in STAT_MEAN_K:
        cases[f"stat_mean_k_{k}"] = (mixture(), _stat(mean_k=k))
    for sd in STAT_STDDEV:
        cases[f"stat_stddev_{sd}"] = (mixture(), _stat(stddev=sd))
    for n in STAT_SIZES:
        cases[f"stat_n_{n}"] = (mixture()[:n], _stat())
    cases["stat_duplicates"] = (duplicates(), _stat(mean_k=2))      # every mean distance is 0 = the threshold: kept by `<=`
    for ds, name in DOWNSAMPLE_NAMES.items():
        cases[f"stat_nonfinite_{name}"] = (nonfinite_mixture(), _stat(downsample=ds))
    cases["radius_nonfinite"] = (nonfinite_mixture(), _radius(2.5, 2))
    for m in RADIUS_MIN_NEIGHBORS:
        cases[f"radius_min_neighbors_{m}"] = (mixture(), _radius(2.5, m))
    for n in RADIUS_SIZES:
        for m in (0, 1):
            cases[f"radius_n_{n}_min_{m}"] = (mixture()[:n], _radius(2.5, m))
    cases["radius_behind_approx"] = (negative_box(), _radius(2.0, 3, downsample=APPROX))
    # behind VoxelGrid, distance filter inline: radius / leaf just above 4 goes to the search tree (k_pf_radius_flags), exactly 4 stays on the voxel grid
    # with G = 16 lanes per centroid (k_pf_grid_radius_flags)
    cases["radius_voxelgrid_tree"] = (negative_box(), _radius(2.001, 3, downsample=VOXELGRID, use_filter=1))
    cases["radius_voxelgrid_grid"] = (negative_box(), _radius(2.0, 3, downsample=VOXELGRID, use_filter=1))
    return cases


# ---- plumbing
def device_params(**fields):
    from hdl_graph_slam_amd import _lib as L
    p = L.HgsPrefilterParams()
    assert L.lib().hgs_prefilter_params_default(C.byref(p)) == L.HGS_OK
    for k, v in fields.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def oracle_params(**fields):
    p = O.default_prefilter_params()
    for k, v in fields.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _engine(make_engine):
    return make_engine(O.default_params(O.HGS_FAST_GICP))


def device_prefilter(reg, cloud, p, **deskew) -> np.ndarray:
    dc = reg.prefilter(cloud, p, **deskew)
    got = dc.download()
    dc.close()
    return np.stack([got["x"], got["y"], got["z"], got["intensity"]], axis=1)


def expect_oracle(reg, cloud, fields, label="", equal_nan=False, **deskew) -> np.ndarray:
    """The device's result is the oracle's: same points, same order, same bits.  Returns it."""
    p = device_params(**fields)
    got = device_prefilter(reg, cloud, p, **deskew)
    ref = O.prefilter(cloud, p, **deskew)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=equal_nan), (label, int((got != ref).any(axis=1).sum()), "points differ")
    return got


def prefilter_status(reg, cloud, fields) -> int:
    """hgs_prefilter's return code for one call (a cloud it returns is released)."""
    from hdl_graph_slam_amd import _lib as L
    p = device_params(**fields)
    arr, n, stride = L.cloud_args(cloud)
    h = C.c_void_p()
    rc = L.lib().hgs_prefilter(reg._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(p), C.byref(h))
    if h:
        L.lib().hgs_cloud_destroy(h)
    return rc


# ---- the outlier filters
def check_outlier_case(make_engine, name):
    cloud, fields = outlier_cases()[name]
    reg = _engine(make_engine)
    got = expect_oracle(reg, cloud, fields, name)
    assert np.isfinite(got[:, :3]).all(), name      # non-finite points are dropped by either outlier filter
    reg.close()
    return got


def check_outlier_cases_are_not_trivial():
    """What the cases are meant to exercise, stated on the oracle's results (no device)."""
    def kept(name):
        cloud, fields = outlier_cases()[name]
        return len(O.prefilter(cloud, oracle_params(**fields))), len(cloud)
    for k in STAT_MEAN_K:
        m, n = kept(f"stat_mean_k_{k}")
        assert 0.5 * n < m < n, (k, m, n)
    assert kept("stat_stddev_0.0")[0] < kept("stat_stddev_1.0")[0] < kept("stat_stddev_2.5")[0] < 600
    assert kept("stat_n_1") == (1, 1) and kept("stat_n_2") == (2, 2)      # d = 0, and two equal d: both AT the threshold
    assert kept("stat_duplicates") == (300, 300)
    m, n = kept("stat_nonfinite_none")
    assert n == 600 and 200 < m < 400                                      # 400 finite points, some of them outliers
    m, n = kept("radius_nonfinite")
    assert 200 < m < 400
    assert kept("radius_min_neighbors_0") == (600, 600)
    assert 0 < kept("radius_min_neighbors_50")[0] < kept("radius_min_neighbors_2")[0] < 600
    for n in RADIUS_SIZES:
        assert kept(f"radius_n_{n}_min_0") == (n, n)
    assert kept("radius_n_1_min_1") == (0, 1)
    for name in ("radius_behind_approx", "radius_voxelgrid_tree", "radius_voxelgrid_grid"):
        m, n = kept(name)
        assert 0 < m < n, (name, m, n)


# ---- voxel grid
def check_voxelgrid_one_long_run(make_engine):
    """3000 points in ONE voxel: a single run of equal keys 12 blocks long (head flags, scan, k_pf_voxel_centroids' ordered float sum)."""
    rng = np.random.default_rng(4)
    cloud = synth.to_xyzi(rng.uniform(0.01, 0.09, (3000, 3)).astype(np.float32) + np.float32([5, 5, 5]), rng.uniform(0, 255, 3000))
    reg = _engine(make_engine)
    got = expect_oracle(reg, cloud, dict(outlier_removal_method=0, downsample_resolution=0.1), "one voxel")
    assert len(got) == 1
    reg.close()


def check_voxelgrid_block_multiples(make_engine):
    """Point counts of exactly one block, one block + 1 and four blocks."""
    reg = _engine(make_engine)
    for n in (256, 257, 1024):
        cloud = mixture(1024, 5)[:n]
        got = expect_oracle(reg, cloud, dict(use_distance_filter=0, outlier_removal_method=0, downsample_resolution=2.0), f"n = {n}")
        assert 0 < len(got) < n
    reg.close()


def check_all_nonfinite_cloud(make_engine):
    """Nothing finite, distance filter off: VoxelGrid and ApproximateVoxelGrid return an empty cloud, and so do the outlier filters on their own."""
    xyz = np.full((70, 3), np.nan, np.float32)
    xyz[1::2, 2] = np.inf
    xyz[1::2, :2] = 1.0
    cloud = synth.to_xyzi(xyz)
    reg = _engine(make_engine)
    for fields in (dict(downsample_method=VOXELGRID, outlier_removal_method=0), dict(downsample_method=APPROX, outlier_removal_method=0),
                   dict(downsample_method=VOXELGRID), dict(downsample_method=NONE, outlier_removal_method=STATISTICAL),
                   dict(downsample_method=NONE, outlier_removal_method=RADIUS)):
        got = expect_oracle(reg, cloud, dict(use_distance_filter=0, **fields), str(fields))
        assert len(got) == 0, fields
    reg.close()


def check_distance_thresholds_are_strict(make_engine):
    """near < |p| < far: a point at exactly distance_near_thresh or distance_far_thresh is dropped, its float neighbours inside are kept — by the flags
    + compaction pass (no downsampling, prefilter_fast = 0) and by the test inside the voxel grid's kernels (prefilter_fast = 1)."""
    one, hundred, inf = np.float32(1.0), np.float32(100.0), np.float32(np.inf)
    xyz = np.array([[1, 0, 0], [100, 0, 0], [0, -1, 0], [0, 0, 100], [np.nextafter(one, inf), 0, 0], [0, np.nextafter(hundred, -inf), 0],
                    [np.nextafter(one, -inf), 0, 0], [0, 0, np.nextafter(hundred, inf)], [3, 4, 0], [0, 60, 80], [0, 6, 8]], np.float32)
    cloud = synth.to_xyzi(xyz, np.arange(len(xyz), dtype=np.float32))
    want = [4.0, 5.0, 8.0, 10.0]      # by intensity: the two inside neighbours, (3, 4, 0) and (0, 6, 8); (0, 60, 80) has |p| = 100 exactly
    for fast in (1, 0):
        reg = _engine(make_engine)
        reg.set_option("prefilter_fast", fast)
        for ds in (VOXELGRID, NONE):
            got = expect_oracle(reg, cloud, dict(downsample_method=ds, downsample_resolution=0.1, outlier_removal_method=0), f"fast {fast} downsample {ds}")
            assert sorted(got[:, 3]) == want, (fast, ds, got[:, 3])
        reg.close()


def check_voxel_index_overflow(make_engine):
    """More than INT_MAX voxels: HGS_ERR_INVALID_ARGUMENT with the "too fine" message, the oracle refuses too, the engine goes on working.  The second
    cloud's 1.2e7 cells per axis wrap a 64-bit product of the three (1.7e21): the comparison must not be made on that product."""
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import HgsError
    reg = _engine(make_engine)
    for span, leaf in ((1500.0, 0.1), (60000.0, 0.01)):
        cloud = synth.to_xyzi(np.array([[-span, -span, -span], [span, span, span], [5, 5, 5]], np.float32))
        fields = dict(use_distance_filter=0, outlier_removal_method=0, downsample_resolution=leaf)
        assert prefilter_status(reg, cloud, fields) == L.HGS_ERR_INVALID_ARGUMENT, (span, leaf)
        assert "too fine" in L.lib().hgs_last_error(reg._h).decode()
        try:
            reg.prefilter(cloud, device_params(**fields))
            raise AssertionError("the overflowing voxel grid was accepted")
        except HgsError as exc:
            assert "too fine" in str(exc)
        try:
            O.prefilter(cloud, oracle_params(**fields))
            raise AssertionError("the oracle accepted the overflowing voxel grid")
        except ValueError:
            pass
        expect_oracle(reg, mixture(), dict(outlier_removal_method=0, downsample_resolution=0.5), "after the refusal")
    # a cloud that just fits is not refused: 1290^3 < 2^31 <= 1291^3 cells
    edge = synth.to_xyzi(np.array([[0.05, 0.05, 0.05], [128.95, 128.95, 128.95]], np.float32))
    assert len(expect_oracle(reg, edge, dict(use_distance_filter=0, outlier_removal_method=0, downsample_resolution=0.1), "1290^3 cells")) == 2
    reg.close()


# ---- approximate voxel grid, deskewing
def check_approx_voxelgrid_edges(make_engine):
    reg = _engine(make_engine)
    base = dict(use_distance_filter=0, outlier_removal_method=0, downsample_method=APPROX)
    one = synth.to_xyzi(np.array([[5.0, -1.0, 0.5]], np.float32), [7.0])
    got = expect_oracle(reg, one, dict(downsample_resolution=0.5, **base), "n = 1")
    assert got.tolist() == [[5.0, -1.0, 0.5, 7.0]]
    # all points in ONE history bucket: voxels (0, 0, 0) and (512, 0, 0) alternate, every point but the first evicts the other voxel
    rng = np.random.default_rng(6)
    xyz = rng.uniform(0.05, 0.95, (300, 3)).astype(np.float32)
    xyz[1::2, 0] += np.float32(512.0)
    bucket = synth.to_xyzi(xyz, rng.uniform(0, 255, 300))
    got = expect_oracle(reg, bucket, dict(downsample_resolution=1.0, **base), "one bucket")
    assert len(got) == 300
    # ... and all points in one voxel: one output
    got = expect_oracle(reg, bucket[0::2], dict(downsample_resolution=1.0, **base), "one voxel")
    assert len(got) == 1
    # negative coordinates (floor, and the hash of negative indices), against the sequential filter
    for leaf in (0.5, 3.0):
        got = expect_oracle(reg, negative_box(), dict(downsample_resolution=leaf, **base), f"negative, leaf {leaf}")
        ref = PR.approx_voxelgrid(negative_box(), leaf)
        assert got.shape == ref.shape and np.array_equal(got, ref), leaf
    reg.close()


def check_deskew_with_a_nonfinite_record(make_engine):
    """A non-finite record in the middle of a deskewed sweep keeps its place (point i turns by scan_period * i / n, n the whole sweep) and stays
    non-finite; the filters behind drop it."""
    cloud = mixture(301, 7).copy()
    cloud["y"][150] = np.nan
    cloud["x"][151] = -np.inf
    imu_w, period = [0.3, -0.2, 1.1], 0.1
    reg = _engine(make_engine)
    got = expect_oracle(reg, cloud, dict(use_distance_filter=0, downsample_method=NONE, outlier_removal_method=0), "deskew only", equal_nan=True,
                        imu_angular_velocity=imu_w, scan_period=period)
    assert len(got) == 301 and not np.isfinite(got[150:152, :3]).all(axis=1).any() and np.isfinite(got[:, :3]).all(axis=1).sum() == 299
    for fields in (dict(downsample_method=NONE), dict(downsample_method=VOXELGRID, downsample_resolution=0.5),
                   dict(downsample_method=APPROX, downsample_resolution=0.5, outlier_removal_method=RADIUS, radius_radius=2.5)):
        got = expect_oracle(reg, cloud, dict(use_distance_filter=0, **fields), str(fields), imu_angular_velocity=imu_w, scan_period=period)
        assert 0 < len(got) < 299
    reg.close()


# ---- arguments
def check_arguments(make_engine):
    from hdl_graph_slam_amd import _lib as L
    reg = _engine(make_engine)
    cloud = mixture()[:80]
    bad = (dict(outlier_removal_method=STATISTICAL, statistical_mean_k=0), dict(outlier_removal_method=STATISTICAL, statistical_mean_k=63),
           dict(outlier_removal_method=STATISTICAL, statistical_mean_k=-1), dict(outlier_removal_method=RADIUS, radius_radius=0.0),
           dict(outlier_removal_method=RADIUS, radius_radius=float("nan")), dict(outlier_removal_method=RADIUS, radius_min_neighbors=-1),
           dict(downsample_method=VOXELGRID, downsample_resolution=0.0), dict(downsample_method=APPROX, downsample_resolution=0.0),
           dict(downsample_method=VOXELGRID, downsample_resolution=float("nan")), dict(downsample_method=3), dict(downsample_method=-1),
           dict(outlier_removal_method=3), dict(outlier_removal_method=-1))
    for fields in bad:
        assert prefilter_status(reg, cloud, fields) == L.HGS_ERR_INVALID_ARGUMENT, fields
    # the parameters of a stage that is off are not looked at
    good = (dict(outlier_removal_method=STATISTICAL, statistical_mean_k=62), dict(outlier_removal_method=RADIUS, statistical_mean_k=0),
            dict(outlier_removal_method=STATISTICAL, radius_radius=0.0, radius_min_neighbors=-1), dict(downsample_method=NONE, downsample_resolution=0.0))
    for fields in good:
        assert prefilter_status(reg, cloud, dict(use_distance_filter=0, **fields)) == L.HGS_OK, fields
    expect_oracle(reg, cloud, dict(use_distance_filter=0, downsample_method=NONE, outlier_removal_method=STATISTICAL, statistical_mean_k=62), "mean_k 62")
    reg.close()
