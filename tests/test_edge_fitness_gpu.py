"""hgs_calc_fitness_score_batch on the MI355X: the shared checks of tests/edge_fitness_checks.py — scores against the single call on fresh
engines bit for bit (FAST_GICP and NDT_OMP engines, with and without seed grids, three ranges), the reference's recorded numbers, the seed tables of
the batched build word for word, handle state, refusals, chunking, the information matrices, and the C++ adapter against the real library."""
import os
import subprocess

import pytest

import edge_fitness_checks as EC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed_grid", [1, 0])
@pytest.mark.parametrize("method", list(EC.METHODS))
def test_batch_scores_equal_the_single_call_on_fresh_engines(method, seed_grid):
    EC.check_scores_equal_single_calls(method, seed_grid)


@pytest.mark.parametrize("method", list(EC.METHODS))
def test_batch_scores_against_the_reference_translation_unit(method):
    EC.check_against_reference_vectors(method)


def test_batched_seed_tables_equal_the_single_cloud_build():
    EC.check_seed_tables()


@pytest.mark.parametrize("method", list(EC.METHODS))
def test_batch_leaves_the_handle_state_alone(method):
    EC.check_handle_state(method)


def test_refusals_write_nothing_and_leave_the_engine_usable():
    EC.check_refusals()


def test_results_do_not_depend_on_the_chunk_size():
    EC.check_chunking()


def test_information_matrices_of_all_edges_equal_the_per_edge_matrices():
    EC.check_information_matrices()


def test_cpp_fitness_scores_equals_fitness_score_per_pair(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    L.lib()                      # (raises when the library has not been built)
    lib = L.LIB_PATH
    exe = os.path.join(ROOT, "tests", "cpp", "edge_fitness_main")
    src_cpp = os.path.join(ROOT, "tests", "cpp", "edge_fitness_main.cpp")
    deps = [src_cpp, os.path.join(ROOT, "adapters", "resident_clouds_hip.hpp"), os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "mock_pcl"),
                        "-I", os.path.join(ROOT, "tests", "mock_eigen"), src_cpp, "-o", exe, "-L", os.path.dirname(lib), "-lhgs_hip",
                        f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    out = subprocess.run([exe, *EC.write_cpp_inputs(tmp_path)], check=True, capture_output=True, text=True).stdout.splitlines()
    EC.check_cpp_output(out)
