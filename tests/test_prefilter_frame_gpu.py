"""The prefilter's base_link transform (hgs_prefilter_framed) on the MI355X: the shared checks of tests/prefilter_frame_checks.py, which
tests/test_prefilter_frame_simt_host.py runs on the host emulation — the transform alone at partly filled waves and blocks, its place behind the
deskewing, the filters behind it, the whole pipeline on one VLP-16 sweep, the calls without a matrix, the refusals, the Python mirror and the C++ adapter."""
import pytest

import prefilter_frame_checks as FC

pytestmark = pytest.mark.gpu


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


def test_frame_cpp_adapter(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    L.lib()
    FC.check_adapter(make, tmp_path, L.LIB_PATH, "prefilter_frame_adapter_main", "hgs_hip")
