"""hgs_prefilter_batch with the outlier removals that need a search tree, on the MI355X: the shared checks of tests/prefilter_batch_tree_checks.py, which
tests/test_prefilter_batch_tree_simt_host.py runs on the host emulation — the batch sequence is taken (two read-backs, one index build, one tree-walk
launch), every out[i] against the single call on a fresh engine bit for bit, the CPU oracle's counts, calls back to back, the handle's state, a failing
call, the outputs in registrations and LockstepOdometry on the nodelet's default outlier removal."""
import pytest

import prefilter_batch_tree_checks as TC

pytestmark = pytest.mark.gpu


def make():
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    return RegistrationHIP(L.default_params(L.HGS_FAST_GICP))


def test_tree_parameter_sets_take_the_batch_sequence():
    TC.check_path_is_taken(make)


@pytest.mark.parametrize("config", sorted(TC.CONFIGS))
def test_tree_batch_equals_single_calls(config):
    TC.check_batch_equals_single_calls(make, config)


def test_mean_k_63_is_refused_by_both():
    TC.check_mean_k_63_is_refused_alike(make)


def test_counts_are_the_oracles():
    TC.check_counts_against_the_oracle(make)


def test_tree_batches_back_to_back():
    TC.check_back_to_back(make)


def test_tree_batch_leaves_the_handle_state_alone():
    TC.check_handle_state(make)


def test_overflow_in_a_tree_batch_leaves_nothing_behind():
    TC.check_overflow_leaves_nothing(make)


def test_tree_batch_outputs_as_sources_and_targets():
    TC.check_downstream_use(make)


def test_lockstep_odometry_on_the_default_outlier_removal():
    TC.check_lockstep_odometry(make)
