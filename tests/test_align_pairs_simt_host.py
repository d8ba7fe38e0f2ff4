"""hgs_align_pairs on the CPU: the product kernels' per-problem-target instantiations (k_ndt_pass, k_vgicp_linearize / k_vgicp_error, and the point
kernels of the grouped call) and the engine's paired batch compiled for the host against the SIMT emulation of tests/emul, through the shared checks
of tests/align_pairs_checks.py — records against single batches bit for bit for all four engines with and without the fitness pass and under every
engine option that selects another path, agreement with hgs_align, handle state, refusals, LoopDetector.detect with reg_hip_batch_pairs,
LockstepOdometry, and the plain C++ caller."""
import os
import subprocess

import pytest

import align_pairs_checks as PC

simt = pytest.importorskip("emul.simt", reason="needs tests/emul")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def simt_library():
    """Points the package's loader at tests/emul/libhgs_simt.so for the duration of this module (and back afterwards)."""
    path = simt.build()
    if path is None:
        pytest.skip("clang++ not available: the emulation build needs ext_vector_type / elementwise builtins")
    from hdl_graph_slam_amd import _lib as L
    saved = (L.LIB_PATH, L._lib)
    L.LIB_PATH, L._lib = path, None
    yield path
    L.LIB_PATH, L._lib = saved


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = PC.Case(name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", ["FAST_GICP", "ICP_HIP_reciprocal", "FAST_VGICP_DIRECT7", "FAST_VGICP_DIRECT27", "NDT_OMP_DIRECT7", "NDT_OMP_KDTREE"])
def test_records_equal_single_batches(cases, name):
    PC.check_records(cases(name))


# (the emulation runs a registration in seconds: the host file takes one engine per path, tests/test_align_pairs_gpu.py every combination)
@pytest.mark.parametrize("name, variant", [("NDT_OMP_DIRECT7", "resident1_chunk2"), ("NDT_OMP_DIRECT7", "resident2_chunk2_lanes4"), ("NDT_OMP_DIRECT1", "resident2_chunk8"),
                                           ("NDT_OMP_KDTREE", "sort0"), ("NDT_OMP_DIRECT7", "sort1")])
def test_ndt_records_under_engine_options(cases, name, variant):
    PC.check_records(cases(name), variant)


@pytest.mark.parametrize("name", ["FAST_VGICP_DIRECT7", "ICP_HIP", "FAST_GICP"])
def test_records_on_four_lanes(cases, name):
    PC.check_records(cases(name), "lanes4")


@pytest.mark.parametrize("name", ["FAST_GICP", "ICP_HIP", "FAST_VGICP_DIRECT7", "NDT_OMP_DIRECT7"])
def test_pairs_agree_with_hgs_align(cases, name):
    PC.check_align_agreement(cases(name))


@pytest.mark.parametrize("name", ["FAST_GICP", "FAST_VGICP_DIRECT7", "NDT_OMP_DIRECT7"])
def test_paired_call_leaves_the_handle_state_alone(cases, name):
    PC.check_handle_state(cases(name))


def test_ndt_calls_of_different_shape_back_to_back(cases):
    PC.check_shapes_back_to_back(cases("NDT_OMP_DIRECT7"))


def test_refusals_leave_the_engine_usable():
    PC.check_refusals()


def test_vgicp_oversized_grid_refuses_the_whole_call(cases):
    PC.check_vgicp_oversized_grid(cases("FAST_VGICP_DIRECT7"))


@pytest.mark.parametrize("method", ["NDT_OMP", "FAST_VGICP"])
def test_detect_through_pairs_equals_the_sequential_detect(method):
    PC.check_detect(method)


@pytest.mark.parametrize("name", ["FAST_GICP", "NDT_OMP_DIRECT7"])
def test_lockstep_odometry_equals_one_odometry_per_stream(name):
    PC.check_lockstep_odometry(name)


@pytest.mark.parametrize("name", PC.CPP_METHODS)
def test_cpp_caller_gives_the_same_records(simt_library, tmp_path, name):
    exe = os.path.join(ROOT, "tests", "cpp", "align_pairs_main_simt")
    src_cpp = os.path.join(ROOT, "tests", "cpp", "align_pairs_main.cpp")
    deps = [src_cpp, os.path.join(ROOT, "include", "hgs_registration.h"), simt_library]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), src_cpp, "-o", exe,
                        "-L", os.path.dirname(simt_library), "-l:libhgs_simt.so", f"-Wl,-rpath,{os.path.dirname(simt_library)}"], check=True)
    out = subprocess.run([exe, *PC.cpp_arguments(name, tmp_path)], check=True, capture_output=True, text=True).stdout.splitlines()
    PC.check_cpp_output(out, name)
