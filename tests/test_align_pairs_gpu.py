"""hgs_align_pairs on the MI355X: the shared checks of tests/align_pairs_checks.py — records against single batches bit for bit for all four engines
with and without the fitness pass and under every engine option that selects another path (lane cuts between targets; for NDT_OMP one or two
resident blocks, so that a block's run crosses problems and targets), agreement with hgs_align, handle state, refusals, LoopDetector.detect with
reg_hip_batch_pairs, LockstepOdometry, and the plain C++ caller against the real library."""
import os
import subprocess

import pytest

import align_pairs_checks as PC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("name", list(PC.METHODS))
def test_records_equal_single_batches(cases, name):
    PC.check_records(cases(name))


@pytest.mark.parametrize("variant", [v for v in PC.NDT_VARIANTS if v != "default"])
@pytest.mark.parametrize("name", ["NDT_OMP_DIRECT1", "NDT_OMP_DIRECT7", "NDT_OMP_KDTREE"])
def test_ndt_records_under_engine_options(cases, name, variant):
    PC.check_records(cases(name), variant)


@pytest.mark.parametrize("name", ["FAST_VGICP_DIRECT1", "FAST_VGICP_DIRECT7", "FAST_VGICP_DIRECT27", "ICP_HIP", "ICP_HIP_reciprocal"])
def test_records_on_four_lanes(cases, name):
    PC.check_records(cases(name), "lanes4")


@pytest.mark.parametrize("variant", [v for v in PC.GICP_VARIANTS if v != "default"])
def test_fast_gicp_records_under_engine_options(cases, variant):
    PC.check_records(cases("FAST_GICP"), variant)


@pytest.mark.parametrize("name", ["FAST_GICP", "ICP_HIP", "FAST_VGICP_DIRECT7", "NDT_OMP_DIRECT7"])
def test_pairs_agree_with_hgs_align(cases, name):
    PC.check_align_agreement(cases(name))


@pytest.mark.parametrize("name", ["FAST_GICP", "ICP_HIP", "FAST_VGICP_DIRECT7", "NDT_OMP_DIRECT7"])
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
def test_cpp_caller_gives_the_same_records(tmp_path, name):
    from hdl_graph_slam_amd import _lib as L
    L.lib()                      # (raises when the library has not been built)
    lib = L.LIB_PATH
    exe = os.path.join(ROOT, "tests", "cpp", "align_pairs_main")
    src_cpp = os.path.join(ROOT, "tests", "cpp", "align_pairs_main.cpp")
    deps = [src_cpp, os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), src_cpp, "-o", exe, "-L", os.path.dirname(lib), "-lhgs_hip",
                        f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    out = subprocess.run([exe, *PC.cpp_arguments(name, tmp_path)], check=True, capture_output=True, text=True).stdout.splitlines()
    PC.check_cpp_output(out, name)
