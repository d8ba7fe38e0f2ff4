"""Floor detection (hgs_detect_floor) on the MI355X against the restatement of tests/floor_reference.py: the shared checks of tests/floor_checks.py
that tests/test_floor_simt_host.py runs on the host emulation, one HDL-64E sweep downsampled at 0.25 m end to end, and the C++ adapter."""
import numpy as np
import pytest

import floor_checks as FC
from hdl_graph_slam_amd import synth

pytestmark = pytest.mark.gpu


def make(pnh=None, **constants):
    from hdl_graph_slam_amd import FloorDetector
    return FloorDetector(pnh, **constants)


def test_floor_clip_tilt_0_is_exact():
    FC.check_clip_tilt0(make)


def test_floor_clip_tilt_3():
    FC.check_clip_tilted(make)


@pytest.mark.parametrize("kind", ["vlp16", "hdl32"])
def test_floor_normal_flags_and_normals(kind):
    FC.check_normals(make, kind)


def test_floor_ransac_counts_hook():
    FC.check_ransac_counts(make)


def test_floor_sequential_rule_and_chunking():
    FC.check_sequential_rule(make)


@pytest.mark.parametrize("kind", ["vlp16", "hdl32"])
def test_floor_end_to_end(kind):
    FC.check_end_to_end(make, kind)


def test_floor_end_to_end_hdl64_sweep():
    cloud = synth.make_pair("HDL-64E", 0, downsample=0.25)[0]
    assert 5000 < len(cloud) <= 35000
    for pnh in ({}, {"use_normal_filtering": False}):
        ref = FC.check_cloud_end_to_end(make, cloud, pnh)
        assert ref.detected


def test_floor_rejection_paths():
    FC.check_rejections(make)


def test_floor_upside_down_scene_gives_an_upward_normal():
    FC.check_upside_down(make)


def test_floor_prefilter_output_goes_in_resident():
    raw = synth.make_pair("VLP-16", 2)[0]
    FC.check_prefilter_output_goes_in_resident(make, raw)


def test_floor_errors():
    from hdl_graph_slam_amd import HgsError
    FC.check_errors(make, HgsError)


def test_floor_python_mirror():
    FC.check_python_mirror(make)


def test_floor_cpp_adapter_matches_the_mirror(tmp_path):
    from hdl_graph_slam_amd import _lib as L
    from floor_adapter_check import check_adapter
    L.lib()
    check_adapter(make, tmp_path, L.LIB_PATH, "floor_adapter_main", "hgs_hip")
