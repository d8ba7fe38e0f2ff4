"""hgs_prefilter_batch with the outlier removals that need a search tree, on the CPU: the k_pfb_* kernels and the engine code that drives them compiled
for the host against the SIMT emulation of tests/emul — the shared checks of tests/prefilter_batch_tree_checks.py, which
tests/test_prefilter_batch_tree_gpu.py runs on the device."""
import pytest

import prefilter_batch_tree_checks as TC

simt = pytest.importorskip("emul.simt", reason="needs tests/emul")


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
