"""ICP_HIP without a GPU: the factory mapping (registrations.cpp:57-64 under the new name), hgs_params_default(HGS_ICP), the restatement of
tests/icp_reference.py on its own (a known rigid motion, the Umeyama step against numpy.linalg.svd including the reflection case), and the
patched factory of the reference compiled against the stand-in headers of tests/mock_* (where the reference tree is present)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import icp_reference as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import integration_build as IB  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from hdl_graph_slam_amd import build
    build.build_lib()
    from hdl_graph_slam_amd import _lib
    _lib.lib()
    return _lib


def test_icp_hip_maps_to_hgs_icp(L):
    from hdl_graph_slam_amd.registrations import params_from_rosparams
    p = params_from_rosparams({"registration_method": "ICP_HIP"})
    assert (p.method, p.transformation_epsilon, p.max_iterations, p.max_correspondence_distance, p.rotation_epsilon) == (L.HGS_ICP, 0.01, 64, 2.5, 0.0)
    assert p.use_reciprocal_correspondences is False and p.reserved == 0
    p = params_from_rosparams({"registration_method": "ICP_HIP", "reg_transformation_epsilon": 0.001, "reg_maximum_iterations": 32,
                               "reg_max_correspondence_distance": 1.5, "reg_use_reciprocal_correspondences": True})
    assert (p.transformation_epsilon, p.max_iterations, p.max_correspondence_distance) == (0.001, 32, 1.5)
    assert p.use_reciprocal_correspondences is True and p.reserved == 1
    assert params_from_rosparams({"registration_method": "ICP_HIP", "reg_use_reciprocal_correspondences": "false"}).use_reciprocal_correspondences is False
    with pytest.raises(NotImplementedError):                 # plain ICP still names PCL's CPU engine
        params_from_rosparams({"registration_method": "ICP"})


def test_params_default_of_icp(L):
    import ctypes as C
    p = L.default_params(L.HGS_ICP)
    assert (p.method, p.max_iterations, p.transformation_epsilon, p.max_correspondence_distance, p.rotation_epsilon, p.reserved) == (3, 64, 0.01, 2.5, 0.0, 0)
    assert L.lib().hgs_params_default(4, C.byref(L.HgsParams())) != 0
    q = L.HgsParams()
    q.use_reciprocal_correspondences = True
    assert q.reserved == 1 and q.use_reciprocal_correspondences


def _rot(rx, ry, rz):
    from hdl_graph_slam_amd import synth
    return synth.pose_matrix([0.0, 0.0, 0.0], [rx, ry, rz])[:3, :3]


def test_umeyama_equals_the_svd_solution():
    rng = np.random.default_rng(3)
    src = rng.normal(0, 5, (200, 3))
    R, t = _rot(0.1, -0.2, 0.7), np.array([1.0, -2.0, 0.5])
    dst = src @ R.T + t
    T = IR.umeyama(src, dst)
    np.testing.assert_allclose(T[:3, :3], R, atol=1e-12)
    np.testing.assert_allclose(T[:3, 3], t, atol=1e-12)
    # the same step from the 17 sums of a pass
    sums = np.concatenate([[len(src)], src.sum(0), dst.sum(0), (dst.T @ src).reshape(9), [0.0]])
    np.testing.assert_allclose(IR.umeyama_from_sums(sums), T, atol=1e-10)
    # reflection: dst is a mirror image of src; Eigen's rule flips the smallest singular direction -> a proper rotation, the one
    # U diag(1, 1, -1) V^T of numpy.linalg.svd
    M = np.diag([1.0, 1.0, -1.0]) @ R
    src2 = rng.normal(0, 1, (100, 3)) * [5.0, 3.0, 0.2]
    dst2 = src2 @ M.T
    T2 = IR.umeyama(src2, dst2)
    assert np.isclose(np.linalg.det(T2[:3, :3]), 1.0)
    S = (dst2 - dst2.mean(0)).T @ (src2 - src2.mean(0)) / len(src2)
    U, _, Vt = np.linalg.svd(S)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    np.testing.assert_allclose(T2[:3, :3], U @ np.diag([1.0, 1.0, -1.0]) @ Vt, atol=1e-12)


def test_reference_recovers_a_known_rigid_motion():
    rng = np.random.default_rng(11)
    # a structured scene: three planes and a pole, 3000 points
    a = rng.uniform(-10, 10, (1000, 2))
    pts = np.concatenate([np.c_[a, np.zeros(1000)], np.c_[a[:, :1], np.full((1000, 1), 8.0), (a[:, 1:] + 10) / 4],
                          np.c_[np.full((500, 1), -7.0), a[:500, :1], (a[:500, 1:] + 10) / 4], np.c_[np.full((500, 2), 2.0), rng.uniform(0, 5, (500, 1))]])
    tgt = pts.astype(np.float32)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(0.01, -0.01, 0.05), [0.3, -0.2, 0.05]
    src = (np.linalg.inv(T)[:3, :3] @ tgt.astype(np.float64).T).T + np.linalg.inv(T)[:3, 3]
    ref = IR.IcpReference(max_iterations=100, transformation_epsilon=1e-10, max_correspondence_distance=2.5)
    ref.setInputTarget(tgt)
    ref.setInputSource(src.astype(np.float32))
    o = ref.align(np.eye(4))
    assert o["converged"] and o["iterations"] > 1
    np.testing.assert_allclose(o["T"], T, atol=1e-5)
    assert o["mse"] < 1e-10


needs_reference = pytest.mark.skipif(not IB.have_reference(), reason="the reference tree is only present in the build container")


@needs_reference
def test_patched_factory_returns_the_icp_engine():
    """The patched src/hdl_graph_slam/registrations.cpp, compiled against tests/mock_* with tests/cpp/icp_factory_main.cpp and linked with the
    host emulation of the library: ICP_HIP returns the HIP adapter with ICP's parameters, plain ICP PCL's CPU engine."""
    from emul import simt
    lib = simt.build()
    if lib is None:
        pytest.skip("clang++ not available")
    with tempfile.TemporaryDirectory() as tmp:
        IB.apply_patch(tmp)
        inc = []
        for d in (os.path.join(ROOT, "tests", "mock_ros"), os.path.join(ROOT, "tests", "mock_pcl"), os.path.join(ROOT, "tests", "mock_eigen"),
                  os.path.join(tmp, "include"), os.path.join(ROOT, "include"), os.path.join(ROOT, "adapters")):
            inc += ["-I", d]
        flags = ["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-DUSE_HGS_HIP", *inc]
        unit, main, exe = os.path.join(tmp, "unit.o"), os.path.join(tmp, "main.o"), os.path.join(tmp, "icp_factory_main")
        subprocess.run([*flags, "-c", os.path.join(tmp, "src", "hdl_graph_slam", "registrations.cpp"), "-o", unit], check=True)
        subprocess.run([*flags, "-c", os.path.join(ROOT, "tests", "cpp", "icp_factory_main.cpp"), "-o", main], check=True)
        libdir = os.path.dirname(lib)
        subprocess.run(["g++", unit, main, "-o", exe, "-L", libdir, "-l:libhgs_simt.so", "-pthread", f"-Wl,-rpath,{libdir}"], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    lines = [ln for ln in out if ln.startswith(("ICP_HIP ", "ICP "))]
    assert lines[0] == ("ICP_HIP hip 1 method 3 max_iterations 64 transformation_epsilon 0.01 rotation_epsilon 0 max_correspondence_distance 2.5 "
                        "reciprocal 0")
    assert lines[1] == ("ICP_HIP hip 1 method 3 max_iterations 32 transformation_epsilon 0.001 rotation_epsilon 0 max_correspondence_distance 1.5 "
                        "reciprocal 1")
    assert lines[2] == "ICP hip 0"
