"""hgs_prefilter_batch on the CPU: the k_pfb_* kernels and the engine code that drives them compiled for the host against the SIMT emulation of
tests/emul, driven through the C-ABI, the Python mirror and the plain C++ caller — the shared checks of tests/prefilter_batch_checks.py, which
tests/test_prefilter_batch_gpu.py runs on the device."""
import pytest

import prefilter_batch_checks as BC

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


def test_cpp_caller(tmp_path, simt_library):
    BC.check_cpp_caller(make, tmp_path, simt_library, "prefilter_batch_main_simt", "hgs_simt")
