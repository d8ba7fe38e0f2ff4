"""hgs_detect_floor_batch on the MI355X: the shared checks of tests/floor_batch_checks.py, which tests/test_floor_batch_simt_host.py runs on the host
emulation — every cloud of every batch against hgs_detect_floor on a fresh engine bit for bit and against tests/floor_reference.py, under both parameter
sets, in both orders, under every chunk and group size, calls back to back, the handle's state, the read-back count, resident input from prefilter_batch,
refusals, the Python mirror, LockstepOdometry with a floor detector and the plain C++ caller."""
import pytest

import floor_batch_checks as BC

pytestmark = pytest.mark.gpu


def make(pnh=None, **constants):
    from hdl_graph_slam_amd import FloorDetector
    return FloorDetector(pnh, **constants)


def test_reference_is_not_trivial():
    BC.check_reference_is_not_trivial()


@pytest.mark.parametrize("reverse", [False, True], ids=["listed", "reversed"])
@pytest.mark.parametrize("params", sorted(BC.PARAM_SETS))
def test_batch_equals_single_calls(params, reverse):
    BC.check_batch_equals_single_calls(make, params, reverse)


def test_chunking_and_grouping_change_nothing():
    BC.check_chunking_and_grouping(make)


def test_repeats_and_calls_back_to_back():
    BC.check_repeats_and_back_to_back(make)


def test_readbacks_do_not_grow_with_the_clouds():
    BC.check_structure(make)


def test_prefilter_batch_output_goes_in_resident():
    BC.check_resident_input(make)


def test_refusals_touch_nothing():
    BC.check_refusals(make)


def test_python_mirror():
    BC.check_python_mirror(make)


def test_lockstep_odometry_detects_floors_in_one_batch():
    BC.check_lockstep_odometry(make)


def test_cpp_caller(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    L.lib()
    BC.check_cpp_caller(make, tmp_path, L.LIB_PATH, "floor_batch_main", "hgs_hip")
