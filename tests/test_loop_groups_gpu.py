"""hgs_loop_match_groups on the MI355X: the shared checks of tests/loop_groups_checks.py — records against per-target batches bit for bit
(FAST_GICP under every engine option that selects another instantiation of its kernels, ICP_HIP, ICP_HIP with reciprocal correspondences),
handle state, refusals, LoopDetector.detect with reg_hip_batch_new_keyframes, and the C++ matcher against the real library."""
import os
import subprocess

import pytest

import loop_groups_checks as GC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = GC.Case(name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("variant", GC.GICP_VARIANTS)
def test_fast_gicp_records_equal_per_target_batches(cases, variant):
    GC.check_records(cases("FAST_GICP"), variant)


@pytest.mark.parametrize("variant", GC.ICP_VARIANTS)
@pytest.mark.parametrize("name", ["ICP_HIP", "ICP_HIP_reciprocal"])
def test_icp_records_equal_per_target_batches(cases, name, variant):
    GC.check_records(cases(name), variant)


@pytest.mark.parametrize("name", ["FAST_GICP", "ICP_HIP"])
def test_grouped_call_leaves_the_handle_state_alone(cases, name):
    GC.check_handle_state(cases(name))


def test_refusals_leave_the_engine_usable():
    GC.check_refusals()


def test_detect_with_batched_new_keyframes_equals_the_sequential_detect():
    GC.check_detect("FAST_GICP")


def test_detect_falls_back_where_the_engine_does_not_serve_groups():
    GC.check_detect_falls_back("NDT_OMP")


def test_cpp_match_groups_equals_match_per_group(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    L.lib()                      # (raises when the library has not been built)
    lib = L.LIB_PATH
    exe = os.path.join(ROOT, "tests", "cpp", "loop_groups_main")
    src_cpp = os.path.join(ROOT, "tests", "cpp", "loop_groups_main.cpp")
    deps = [src_cpp, os.path.join(ROOT, "adapters", "loop_match_hip.hpp"), os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), src_cpp, "-o", exe, "-L", os.path.dirname(lib), "-lhgs_hip",
                        f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    out = subprocess.run([exe, "0", "1", *GC.write_cpp_inputs(tmp_path)], check=True, capture_output=True, text=True).stdout.splitlines()
    GC.check_cpp_output(out)
