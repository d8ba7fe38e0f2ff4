"""Floor detection (hgs_detect_floor: k_floor_clip_flags, k_knn_cov's staging mode + k_floor_normal_flags, k_floor_ransac_planes / _count / _decide,
k_floor_inlier_flags and the engine code that drives them) on the CPU: the product sources compiled for the host against the SIMT emulation of
tests/emul, driven through the C-ABI and the Python mirror, against the restatement of tests/floor_reference.py — the shared checks of
tests/floor_checks.py, which tests/test_floor_gpu.py runs on the device."""
import os
import subprocess

import numpy as np
import pytest

import floor_checks as FC
from hdl_graph_slam_amd import synth

simt = pytest.importorskip("emul.simt", reason="needs tests/emul")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def test_floor_rejection_paths():
    FC.check_rejections(make)


def test_floor_upside_down_scene_gives_an_upward_normal():
    FC.check_upside_down(make)


def test_floor_prefilter_output_goes_in_resident():
    raw = synth.make_pair("VLP-16", 2)[0]                   # a raw sweep through the device prefilter (the nodelet's defaults)
    FC.check_prefilter_output_goes_in_resident(make, raw)


def test_floor_errors():
    from hdl_graph_slam_amd import HgsError
    FC.check_errors(make, HgsError)


def test_floor_python_mirror():
    FC.check_python_mirror(make)


def test_floor_cpp_adapter_matches_the_mirror(tmp_path, simt_library):
    from floor_adapter_check import check_adapter
    check_adapter(make, tmp_path, simt_library, "floor_adapter_main_simt", "hgs_simt")
