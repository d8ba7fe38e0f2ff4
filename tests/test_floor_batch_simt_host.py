"""hgs_detect_floor_batch on the CPU: the k_flb_* kernels and the engine code that drives them compiled for the host against the SIMT emulation of
tests/emul, driven through the C-ABI, the Python mirror and the plain C++ caller — the shared checks of tests/floor_batch_checks.py, which
tests/test_floor_batch_gpu.py runs on the device."""
import pytest

import floor_batch_checks as BC

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


def test_cpp_caller(tmp_path, simt_library):
    BC.check_cpp_caller(make, tmp_path, simt_library, "floor_batch_main_simt", "hgs_simt")
