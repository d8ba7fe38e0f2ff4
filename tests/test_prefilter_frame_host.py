"""Host-only checks of the base_link transform's yardstick (no library under test): tests/prefilter_frame_reference.py against the mock
pcl::transformPointCloud of tests/mock_pcl (PCL >= 1.10's order) compiled with -ffp-contract=off — tests/cpp/prefilter_frame_pcl_main.cpp — bit for bit, on
points that include large coordinates, subnormals, signed zeros and non-finite rows; and the properties of the inputs the device checks rely on."""
import os
import subprocess

import numpy as np

import prefilter_frame_checks as FC
import prefilter_frame_reference as PFR
from hdl_graph_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pcl_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "prefilter_frame_pcl_main")
    src = os.path.join(ROOT, "tests", "cpp", "prefilter_frame_pcl_main.cpp")
    deps = [src, os.path.join(ROOT, "tests", "mock_pcl", "pcl", "common", "transforms.h"), os.path.join(ROOT, "tests", "mock_pcl", "pcl", "point_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "mock_pcl"), "-I", os.path.join(ROOT, "tests", "mock_eigen"),
                        src, "-o", exe], check=True)
    return exe


def _points():
    """4000 records: a scene-sized cloud, coordinates up to 1e37 and 3e38 on one axis, subnormals, signed zeros, non-finite rows.  Nothing overflows to
    opposite infinities, so the transform itself produces no NaN."""
    rng = np.random.default_rng(21)
    xyz = rng.normal(0, 30, (4000, 3)).astype(np.float32)
    xyz[500:800] *= np.float32(10.0) ** rng.integers(5, 37, (300, 1)).astype(np.float32)                 # 1e5 ... 1e37
    xyz[800:900] = 0
    xyz[np.arange(800, 900), rng.integers(0, 3, 100)] = np.float32(3e38) * rng.choice(np.float32([-1, 1]), 100)      # 3e38 on one axis, 0 elsewhere
    sub = rng.integers(1, 1 << 23, (300, 3)).astype(np.uint32) | (rng.integers(0, 2, (300, 3)).astype(np.uint32) << 31)
    xyz[900:1200] = sub.view(np.float32)                                                                  # subnormals of either sign
    xyz[1200:1300] = rng.choice(np.float32([0.0, -0.0, 1.0, -2.5]), (100, 3))                             # +-0 in every position
    xyz[1300:1320] = np.float32([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]] * 10)
    bad = rng.choice(np.float32([np.nan, np.inf, -np.inf]), 300)
    xyz[np.arange(1400, 1700), rng.integers(0, 3, 300)] = bad                                             # non-finite rows
    xyz[1700:1710] = np.nan
    return synth.to_xyzi(xyz, rng.uniform(0, 255, 4000))


def test_reference_equals_the_mock_pcl_transform(tmp_path):
    exe = _pcl_exe()
    cloud = _points()
    xyz = synth.xyz_of(cloud)
    finite = np.isfinite(xyz).all(axis=1)
    sub = (np.abs(xyz) < np.finfo(np.float32).tiny) & (xyz != 0)
    assert (~finite).sum() >= 300 and sub.any(axis=1).sum() >= 300 and (np.abs(xyz[finite]) > 1e30).any() and (np.signbit(xyz) & (xyz == 0)).sum() > 50
    cloud.tofile(tmp_path / "c.bin")
    odd = np.array([[2.0, 0.5, 0.0, 1.0], [0.0, -3.0, 0.25, 0.0], [1e-3, 0.0, 0.5, -2.0], [0.0, 0.0, 0.0, 1.0]])
    small = PFR.rigid([0.0, 0.0, 1.0], 1e-3, [1e-40, 0.0, -1e-42])           # subnormal translation entries
    for k, T in enumerate((FC.T_GENERAL, np.eye(4), PFR.rigid([0.0, 0.0, 1.0], np.pi / 2, [0.0, 0.0, 0.0]), small, odd)):
        m = PFR.matrix32(T)
        np.ascontiguousarray(m.T).tofile(tmp_path / f"m{k}.bin")             # column-major
        subprocess.run([exe, str(tmp_path / "c.bin"), str(tmp_path / f"m{k}.bin"), str(tmp_path / f"o{k}.bin")], check=True, capture_output=True)
        want = np.fromfile(tmp_path / f"o{k}.bin", dtype=synth.POINT_XYZI_DTYPE)
        got = PFR.transform(cloud, T)
        FC.same_bits(got, want, k)
        assert np.array_equal(got["w"], want["w"]) and (want["w"] == 1.0).all()          # PCL's fourth lane stays 1 for a bottom row of 0 0 0 1
        assert np.array_equal(FC.bits(got)[~finite], FC.bits(cloud)[~finite])            # non-finite rows pass untouched, NaN payloads included
        assert not np.isnan(synth.xyz_of(got)[finite]).any()
    # the order matters to the last bit: PCL 1.8's left-to-right sum differs from it on this cloud (the stated deviation of DESIGN.md)
    m = PFR.matrix32(FC.T_GENERAL)
    x, y, z = xyz[finite, 0], xyz[finite, 1], xyz[finite, 2]
    with np.errstate(all="ignore"):
        pcl18 = ((m[0, 0] * x + m[0, 1] * y) + m[0, 2] * z) + m[0, 3]
    assert (pcl18 != PFR.transform_xyz(xyz[finite], FC.T_GENERAL)[:, 0]).mean() > 0.05


def test_reference_rounds_every_operation_to_float():
    """One point worked by hand: each product and sum rounded to float32 on its own (no double intermediate, no fused multiply-add)."""
    f = np.float32
    T = np.array([[0.1, 0.7, -0.3, 1e-3], [0.3, 0.1, 0.9, 5.0], [-0.9, 0.2, 0.1, -7.0], [0, 0, 0, 1]])
    m = PFR.matrix32(T)
    p = f([12345.678, -0.001234, 987.654])
    want = [f(f(p[0] * m[r, 0]) + f(f(p[1] * m[r, 1]) + f(f(p[2] * m[r, 2]) + m[r, 3]))) for r in range(3)]
    got = PFR.transform_xyz(p[None, :], T)[0]
    assert got.tolist() == [float(v) for v in want]
    exact = T[:3, :3].astype(np.float32).astype(np.float64) @ p.astype(np.float64) + m[:3, 3].astype(np.float64)
    assert (got.astype(np.float64) != exact).any() and np.allclose(got, exact, rtol=1e-5)


def test_inputs_of_the_device_checks():
    T = FC.T_GENERAL
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(T[:3, :3]), 1.0) and (np.abs(T[:3, :3]) > 0.05).all()
    assert T[3].tolist() == [0, 0, 0, 1] and 2 < np.linalg.norm(T[:3, 3]) < 10
    g, s = FC.general_cloud(), FC.special_cloud()
    assert len(g) == len(s) == max(FC.LOAD_SIZES) == 513 and not g.flags.writeable and not s.flags.writeable
    xyz = synth.xyz_of(s)
    assert not np.isfinite(xyz[0]).all() and (np.signbit(xyz) & (xyz == 0)).any() and ((np.abs(xyz) < np.finfo(np.float32).tiny) & (xyz != 0)).any()
    assert not np.isnan(synth.xyz_of(PFR.transform(s, T))[np.isfinite(xyz).all(axis=1)]).any()        # the transform produces no NaN of its own
