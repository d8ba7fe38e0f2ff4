"""hgs_prefilter_batch on the MI355X: the shared checks of tests/prefilter_batch_checks.py, which tests/test_prefilter_batch_simt_host.py runs on the host
emulation — every out[i] against the single call on a fresh engine bit for bit under every parameter set that takes another path, calls back to back, the
handle's state, refusals, a voxel grid that overflows, the outputs in registrations, LockstepOdometry with prefilter_params and the plain C++ caller."""
import pytest

import prefilter_batch_checks as BC

pytestmark = pytest.mark.gpu


def make():
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    return RegistrationHIP(L.default_params(L.HGS_FAST_GICP))


def test_reference_is_not_trivial():
    BC.check_reference_is_not_trivial()


@pytest.mark.parametrize("config", sorted(BC.CONFIGS))
def test_batch_equals_single_calls(config):
    BC.check_batch_equals_single_calls(make, config)


def test_one_sweep_and_no_sweep():
    BC.check_one_sweep(make)


def test_calls_of_different_shape_back_to_back():
    BC.check_back_to_back(make)


def test_batch_leaves_the_handle_state_alone():
    BC.check_handle_state(make)


def test_refusals_touch_nothing():
    BC.check_refusals(make)


@pytest.mark.parametrize("config", ["vg010_none", "statistical", "slow_vg025_none"])
def test_voxel_grid_overflow_fails_the_whole_call(config):
    BC.check_voxel_grid_overflow(make, config)


def test_outputs_as_sources_and_targets():
    BC.check_downstream_use(make)


def test_lockstep_odometry_prefilters_in_one_batch():
    BC.check_lockstep_odometry(make)


def test_cpp_caller(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    L.lib()
    BC.check_cpp_caller(make, tmp_path, L.LIB_PATH, "prefilter_batch_main", "hgs_hip")
