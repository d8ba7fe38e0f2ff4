"""Shared checks of the prefilter's base_link transform (hgs_prefilter_framed: k_pf_load<true> of hgs_kernels.hip, pf_transform_point of hgs_math.h, the
argument handling of prefilter_impl in hgs_engine.hip, the Python mirror and adapters/resident_clouds_hip.hpp).  tests/test_prefilter_frame_gpu.py runs
them on the MI355X, tests/test_prefilter_frame_simt_host.py on the host emulation of the same kernels.  `make_engine()` builds a RegistrationHIP on the
library under test.

The yardstick is tests/prefilter_frame_reference.py (pcl::transformPointCloud's float arithmetic in numpy).  Every comparison is of BITS: the arithmetic is
fixed and no sum is re-associated, so there is no tolerance.  Most checks compare two device outputs — hgs_prefilter_framed(x, T) against hgs_prefilter of
the host-transformed x — which keeps them independent of what the later stages do with a non-finite point."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

import oracle as O
import prefilter_checks as PFC
import prefilter_frame_reference as PFR
from hdl_graph_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, VOXELGRID, APPROX = 0, 1, 2       # HGS_DOWNSAMPLE_*
STATISTICAL, RADIUS = 1, 2              # HGS_OUTLIER_*
NO_FILTERS = dict(use_distance_filter=0, downsample_method=NONE, outlier_removal_method=NONE)
LOAD_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)      # partly filled waves (64 lanes) and blocks (256 threads) of k_pf_load

# rotation by 0.7 rad about the skew axis (1, 2, 3), translation of a few metres
T_GENERAL = PFR.rigid([1.0, 2.0, 3.0], 0.7, [2.5, -1.25, 3.75])
IMU_W, SCAN_PERIOD = [0.3, -0.2, 1.1], 0.1          # 0.11 rad over the sweep: the last points of a 30 m return move by metres, those at 1 m by centimetres


# ---- inputs (computed once, read-only)
@functools.lru_cache(maxsize=None)
def general_cloud() -> np.ndarray:
    cloud = PFC.mixture(513, 11)
    xyz = synth.xyz_of(cloud)
    assert np.isfinite(xyz).all() and not (np.signbit(xyz) & (xyz == 0)).any()        # finite, and no -0.0 (check_nothing_existing_moved)
    return cloud


@functools.lru_cache(maxsize=None)
def special_cloud() -> np.ndarray:
    """The general cloud with non-finite rows (NaN and either infinity, in every coordinate; row 0 among them, so that n = 1 is one), signed zeros,
    subnormals and coordinates of 1e30.  No input makes the transform itself produce a NaN (its sign differs between processors)."""
    cloud = general_cloud().copy()
    i = np.arange(len(cloud))
    cloud["x"][i % 7 == 0] = np.nan
    cloud["y"][i % 11 == 5] = -np.inf
    cloud["z"][i % 13 == 6] = np.inf
    cloud["z"][i % 29 == 9] = np.nan
    tiny = np.float32(1e-41)
    for k, row in ((1, (0.0, 0.0, 0.0)), (2, (-0.0, -0.0, -0.0)), (8, (0.0, -0.0, 1.0)), (15, (tiny, -tiny, tiny)), (16, (-tiny, 0.0, -0.0)),
                   (62, (1e30, -1e30, 1e30)), (65, (-1e30, 2.0, -3.0)), (254, (tiny, 1e30, -0.0)), (257, (-0.0, tiny, 5.0)), (512, (1e30, 1e30, 1e30))):
        cloud["x"][k], cloud["y"][k], cloud["z"][k] = row
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def sweep() -> np.ndarray:
    """One synthetic VLP-16 revolution in firing order, with intensities."""
    cloud = synth.scan(synth.make_scene(3), "VLP-16", synth.pose_matrix([0, 0, 0], [0, 0, 0]), 103)
    cloud["intensity"] = np.random.default_rng(3).uniform(0, 255, len(cloud)).astype(np.float32)
    cloud.setflags(write=False)
    return cloud


# ---- plumbing
def bits(records: np.ndarray) -> np.ndarray:
    """[n, 4] uint32: the bit patterns of x, y, z, intensity."""
    return np.stack([np.ascontiguousarray(records[f]).view(np.uint32) for f in ("x", "y", "z", "intensity")], axis=1)


def same_bits(a: np.ndarray, b: np.ndarray, label="") -> None:
    assert len(a) == len(b), (label, len(a), len(b))
    ba, bb = bits(a), bits(b)
    assert np.array_equal(ba, bb), (label, int((ba != bb).any(axis=1).sum()), "of", len(a), "points differ")


def prefilter(reg, cloud, p, **kw) -> np.ndarray:
    """The Python mirror: hgs_prefilter / hgs_prefilter_deskewed (/ hgs_prefilter_framed with base_link_transform), downloaded as records."""
    dc = reg.prefilter(cloud, p, **kw)
    out = dc.download()
    dc.close()
    return out


def framed_status(reg, cloud, p, w=None, scan_period=SCAN_PERIOD, colmajor=None):
    """hgs_prefilter_framed itself (either pointer may be NULL): (status, downloaded records or None)."""
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import DeviceCloud
    arr, n, stride = L.cloud_args(cloud)
    wv = None if w is None else np.ascontiguousarray(w, np.float64).reshape(3)
    m = None if colmajor is None else np.ascontiguousarray(colmajor, np.float32).reshape(16)
    h = C.c_void_p()
    rc = L.lib().hgs_prefilter_framed(reg._h, arr.ctypes.data_as(C.c_void_p), n, stride, C.byref(p), None if wv is None else wv.ctypes.data_as(C.c_void_p),
                                      float(scan_period), None if m is None else L.fptr(m), C.byref(h))
    if rc != L.HGS_OK:
        assert not h
        return rc, None
    dc = DeviceCloud._adopt(reg, h)
    out = dc.download()
    dc.close()
    return rc, out


def framed(reg, cloud, p, w=None, T=None, scan_period=SCAN_PERIOD) -> np.ndarray:
    from hdl_graph_slam_amd import _lib as L
    rc, out = framed_status(reg, cloud, p, w, scan_period, None if T is None else L.colmajor16(T))
    assert rc == L.HGS_OK, (rc, L.lib().hgs_last_error(reg._h))
    return out


# ---- 1. the transform alone
def check_transform_alone(make_engine):
    reg = make_engine()
    p = PFC.device_params(**NO_FILTERS)
    for name, cloud in (("general", general_cloud()), ("special", special_cloud())):
        for n in LOAD_SIZES:
            x = cloud[:n]
            got = framed(reg, x, p, T=T_GENERAL)
            want = PFR.transform(x, T_GENERAL)
            same_bits(got, prefilter(reg, want, p), (name, n))
            same_bits(got, want, (name, n, "reference"))              # with every filter off the output IS the transformed input
            if name == "general":
                assert not np.array_equal(bits(got)[:, :3], bits(x)[:, :3]) and np.array_equal(bits(got)[:, 3], bits(x)[:, 3]), n
    sp = special_cloud()
    moved = PFR.transform(sp, T_GENERAL)
    bad = ~np.isfinite(synth.xyz_of(sp)).all(axis=1)
    assert 100 < bad.sum() < 200 and np.array_equal(bits(moved)[bad], bits(sp)[bad])          # the non-finite rows pass untouched
    empty = general_cloud()[:0]
    assert len(framed(reg, empty, p, T=T_GENERAL)) == len(prefilter(reg, empty, p)) == 0
    assert len(framed(reg, empty, PFC.device_params(), w=IMU_W, T=T_GENERAL)) == len(prefilter(reg, empty, PFC.device_params())) == 0
    reg.close()


# ---- 2. the order: deskewing, then the transform
def check_order(make_engine):
    reg = make_engine()
    p = PFC.device_params(**NO_FILTERS)
    for cloud in (general_cloud(), special_cloud()):
        got = framed(reg, cloud, p, w=IMU_W, T=T_GENERAL)
        deskewed = prefilter(reg, cloud, p, imu_angular_velocity=IMU_W, scan_period=SCAN_PERIOD)
        same_bits(got, prefilter(reg, PFR.transform(deskewed, T_GENERAL), p), "deskew, then transform")
        other = prefilter(reg, PFR.transform(cloud, T_GENERAL), p, imu_angular_velocity=IMU_W, scan_period=SCAN_PERIOD)
        ok = np.isfinite(synth.xyz_of(got)).all(axis=1) & np.isfinite(synth.xyz_of(other)).all(axis=1)
        d = np.linalg.norm(synth.xyz_of(got)[ok].astype(np.float64) - synth.xyz_of(other)[ok].astype(np.float64), axis=1)
        d = d[d < 1e20]
        assert np.median(d) > 0.01, np.median(d)       # the other order puts the points centimetres and more away: the check above can tell the two apart
    reg.close()


# ---- 3. the filters see the base frame
def check_filters_see_the_base_frame(make_engine):
    T = np.eye(4)
    T[0, 3] = 0.3
    cloud = synth.to_xyzi(np.array([[0.9, 0.0, 0.0], [-1.1, 0.0, 0.0]], np.float32), [7.0, 9.0])
    for fast in (1, 0):
        reg = make_engine()
        reg.set_option("prefilter_fast", fast)
        for ds in (NONE, VOXELGRID):
            p = PFC.device_params(use_distance_filter=1, distance_near_thresh=1.0, downsample_method=ds, downsample_resolution=0.1, outlier_removal_method=NONE)
            got = framed(reg, cloud, p, T=T)
            assert got["intensity"].tolist() == [7.0], (fast, ds, got)           # 0.9 m from the sensor, 1.2 m from base_link: kept
            same_bits(got, PFR.transform(cloud, T)[:1], (fast, ds))
            assert prefilter(reg, cloud, p)["intensity"].tolist() == [9.0], (fast, ds)      # (1.1 m from the sensor, 0.8 m from base_link: dropped above)
        reg.close()


# ---- 4. the whole pipeline
PIPELINES = {"radius": dict(outlier_removal_method=RADIUS), "approx": dict(downsample_method=APPROX)}


@functools.lru_cache(maxsize=None)
def host_deskewed_transformed_sweep() -> np.ndarray:
    raw = sweep()
    d = O.prefilter(raw, PFC.device_params(**NO_FILTERS), imu_angular_velocity=IMU_W, scan_period=SCAN_PERIOD)       # the oracle's deskewing, nothing else
    assert d.shape == (len(raw), 4) and np.array_equal(d[:, 3], raw["intensity"])
    out = PFR.transform(synth.to_xyzi(d[:, :3], d[:, 3]), T_GENERAL)
    out.setflags(write=False)
    return out


def check_pipeline(make_engine, name, fast):
    raw, want_in = sweep(), host_deskewed_transformed_sweep()
    assert 10000 < len(raw) < 40000
    p = PFC.device_params(**PIPELINES[name])            # the nodelet's defaults otherwise
    reg = make_engine()
    reg.set_option("prefilter_fast", fast)
    got = framed(reg, raw, p, w=IMU_W, T=T_GENERAL)
    want = prefilter(reg, want_in, p)
    assert 1000 < len(want) < len(raw)
    same_bits(got, want, (name, fast))
    reg.close()
    return got


def check_prefilter_fast_gives_the_same_bits(make_engine):
    """Both values of the `prefilter_fast` option: the distance filter inside the voxel grid's kernels or in a pass of its own, RadiusOutlierRemoval on the
    voxel grid (radius / leaf <= 4) or on the search tree — behind the transform the same points come out."""
    raw = sweep()
    for fields in (dict(outlier_removal_method=RADIUS), dict(outlier_removal_method=RADIUS, radius_radius=0.4)):
        out = []
        for fast in (0, 1):
            reg = make_engine()
            reg.set_option("prefilter_fast", fast)
            out.append(framed(reg, raw, PFC.device_params(**fields), w=IMU_W, T=T_GENERAL))
            reg.close()
        assert len(out[0]) > 1000
        same_bits(out[0], out[1], fields)


# ---- 5. nothing existing moved
def check_nothing_existing_moved(make_engine):
    reg = make_engine()
    for cloud in (general_cloud(), special_cloud()):
        for fields in (NO_FILTERS, dict(downsample_resolution=0.5, outlier_removal_method=RADIUS, radius_radius=2.5), dict(downsample_method=APPROX, downsample_resolution=0.5)):
            p = PFC.device_params(**fields)
            same_bits(framed(reg, cloud, p, w=IMU_W, T=None), prefilter(reg, cloud, p, imu_angular_velocity=IMU_W, scan_period=SCAN_PERIOD), ("no matrix", fields))
            same_bits(framed(reg, cloud, p, w=None, T=None), prefilter(reg, cloud, p), ("no matrix, no gyro sample", fields))
    # the identity: the same VALUES (-0.0 + 0.0 is +0.0, so not the same bits for every input; general_cloud() has no -0.0)
    for fields in (NO_FILTERS, dict(downsample_resolution=0.5)):
        p = PFC.device_params(**fields)
        a, b = framed(reg, general_cloud(), p, T=np.eye(4)), prefilter(reg, general_cloud(), p)
        assert len(a) == len(b) > 0 and all((a[f] == b[f]).all() for f in ("x", "y", "z", "intensity")), fields
    reg.close()


# ---- 6. refusals
def check_refusals(make_engine):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import HgsError
    reg = make_engine()
    p = PFC.device_params(**NO_FILTERS)
    cloud = general_cloud()[:100]
    good = L.colmajor16(T_GENERAL)
    want = PFR.transform(cloud, T_GENERAL)
    nan_entry, inf_entry, bottom_2, bottom_x = good.copy(), good.copy(), good.copy(), good.copy()
    nan_entry[5], inf_entry[12], bottom_2[15], bottom_x[3] = np.nan, np.inf, 2.0, 1e-3
    for m, text in ((nan_entry, "non-finite"), (inf_entry, "non-finite"), (bottom_2, "bottom row"), (bottom_x, "bottom row")):
        rc, out = framed_status(reg, cloud, p, colmajor=m)
        assert rc == L.HGS_ERR_INVALID_ARGUMENT and out is None, (text, rc)
        assert text in L.lib().hgs_last_error(reg._h).decode(), (text, L.lib().hgs_last_error(reg._h))
        rc, out = framed_status(reg, cloud, p, w=IMU_W, colmajor=m)
        assert rc == L.HGS_ERR_INVALID_ARGUMENT, (text, rc)
        same_bits(framed(reg, cloud, p, T=T_GENERAL), want, "after the refusal: " + text)        # the engine stays usable
    try:
        reg.prefilter(cloud, p, base_link_transform=bottom_2.reshape(4, 4).T)
        raise AssertionError("the mirror accepted a bottom row of 0 0 0 2")
    except HgsError as exc:
        assert "bottom row" in str(exc)
    # the rotation block is not checked (pcl::transformPointCloud does not check it either): a scaling, shearing matrix is applied as it is
    odd = np.array([[2.0, 0.5, 0.0, 1.0], [0.0, -3.0, 0.25, 0.0], [0.0, 0.0, 0.5, -2.0], [0.0, 0.0, 0.0, 1.0]])
    same_bits(framed(reg, cloud, p, T=odd), PFR.transform(cloud, odd), "not orthogonal")
    assert framed_status(reg, cloud, p, w=IMU_W, scan_period=float("nan"), colmajor=good)[0] == L.HGS_ERR_INVALID_ARGUMENT
    same_bits(framed(reg, cloud, p, T=T_GENERAL), want, "after the refusals")
    reg.close()


# ---- the Python mirror
def check_python_mirror(make_engine):
    """Registration.prefilter(base_link_transform = a row-major 4x4) is hgs_prefilter_framed with the transposed floats; None makes the calls of before."""
    reg = make_engine()
    cloud = special_cloud()
    for fields in (NO_FILTERS, dict(downsample_resolution=0.5, outlier_removal_method=RADIUS, radius_radius=2.5)):
        p = PFC.device_params(**fields)
        for w in (None, IMU_W):
            got = prefilter(reg, cloud, p, imu_angular_velocity=w, scan_period=SCAN_PERIOD, base_link_transform=T_GENERAL)
            same_bits(got, framed(reg, cloud, p, w=w, T=T_GENERAL), ("mirror", fields, w))
            got = prefilter(reg, cloud, p, imu_angular_velocity=w, scan_period=SCAN_PERIOD, base_link_transform=T_GENERAL.astype(np.float32).tolist())
            same_bits(got, framed(reg, cloud, p, w=w, T=T_GENERAL), ("mirror, nested lists", fields, w))
            same_bits(prefilter(reg, cloud, p, imu_angular_velocity=w, scan_period=SCAN_PERIOD, base_link_transform=None), framed(reg, cloud, p, w=w, T=None), ("None", fields, w))
    p = PFC.device_params(**NO_FILTERS)
    same_bits(prefilter(reg, general_cloud(), p, base_link_transform=T_GENERAL), PFR.transform(general_cloud(), T_GENERAL), "row-major in, not transposed twice")
    reg.close()


# ---- 7. the C++ adapter
def fnv1a(records: np.ndarray) -> int:
    h = 1469598103934665603
    for byte in bits(records).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def build_adapter(lib: str, exe_name: str, link_name: str) -> str:
    exe = os.path.join(ROOT, "tests", "cpp", exe_name)
    src = os.path.join(ROOT, "tests", "cpp", "prefilter_frame_adapter_main.cpp")
    deps = [src, os.path.join(ROOT, "adapters", "resident_clouds_hip.hpp"), os.path.join(ROOT, "include", "hgs_registration.h"),
            os.path.join(ROOT, "tests", "mock_pcl", "pcl", "common", "transforms.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "mock_pcl"), "-I", os.path.join(ROOT, "tests", "mock_eigen"),
                        "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-l" + link_name, f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    return exe


def check_adapter(make_engine, tmp_path, lib, exe_name, link_name):
    """ResidentCloudsHIP::prefilter with the matrix against the same call on the sweep the mock pcl::transformPointCloud moved on the host (no matrix):
    identical; and the first against the Python mirror on the same library."""
    from hdl_graph_slam_amd import _lib as L
    exe = build_adapter(lib, exe_name, link_name)
    raw = sweep()
    raw.tofile(tmp_path / "raw.bin")
    L.colmajor16(T_GENERAL).tofile(tmp_path / "m.bin")
    out = subprocess.run([exe, str(tmp_path / "raw.bin"), str(tmp_path / "m.bin"), str(VOXELGRID), str(RADIUS)], check=True, capture_output=True, text=True).stdout.split()
    rec = {out[i]: out[i + 1] for i in range(0, len(out), 2)}
    assert int(rec["raw"]) == len(raw) and int(rec["device_calls"]) == 2, rec
    assert rec["identical"] == "1" and rec["framed"] == rec["host_transformed"], rec
    reg = make_engine()
    got = prefilter(reg, raw, PFC.device_params(outlier_removal_method=RADIUS), base_link_transform=T_GENERAL)
    assert 1000 < len(got) == int(rec["framed"]) and f"{fnv1a(got):016x}" == rec["checksum"], rec
    reg.close()
