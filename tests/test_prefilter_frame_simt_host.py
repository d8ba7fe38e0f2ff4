"""The prefilter's base_link transform (hgs_prefilter_framed: k_pf_load<true>, pf_transform_point and the engine code that drives them) on the CPU: the
product sources compiled for the host against the SIMT emulation of tests/emul, driven through the C-ABI, the Python mirror and the C++ adapter — the
shared checks of tests/prefilter_frame_checks.py, which tests/test_prefilter_frame_gpu.py runs on the device."""
import pytest

import prefilter_frame_checks as FC

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


def test_frame_transform_alone():
    FC.check_transform_alone(make)


def test_frame_deskewing_comes_first():
    FC.check_order(make)


def test_frame_filters_see_the_base_frame():
    FC.check_filters_see_the_base_frame(make)


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("name", sorted(FC.PIPELINES))
def test_frame_whole_pipeline(name, fast):
    FC.check_pipeline(make, name, fast)


def test_frame_prefilter_fast_gives_the_same_bits():
    FC.check_prefilter_fast_gives_the_same_bits(make)


def test_frame_nothing_existing_moved():
    FC.check_nothing_existing_moved(make)


def test_frame_refusals():
    FC.check_refusals(make)


def test_frame_python_mirror():
    FC.check_python_mirror(make)


def test_frame_cpp_adapter(tmp_path, simt_library):
    FC.check_adapter(make, tmp_path, simt_library, "prefilter_frame_adapter_main_simt", "hgs_simt")
