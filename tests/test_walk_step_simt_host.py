"""The quad walks' bookkeeping on the CPU: the product kernels compiled for the host against the SIMT emulation of tests/emul (which aborts on a
wave operation outside wave-uniform control flow), through the shared checks of tests/walk_step_checks.py."""
import pytest

import walk_step_checks as WC

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


def _engine(params):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    p = L.HgsParams()
    for name, _ in L.HgsParams._fields_:
        setattr(p, name, getattr(params, name))
    return RegistrationHIP(p)


@pytest.mark.parametrize("n", WC.TARGET_SIZES)
def test_nn1_walks_on_random_targets(n):
    WC.check_random_target(_engine, n)


def test_nn1_walks_on_a_regular_grid():
    WC.check_grid_target(_engine)


@pytest.mark.parametrize("gather_mode", ["0", "1", "2"])
@pytest.mark.parametrize("n", [2049, 8193])
def test_covariances(n, gather_mode):
    WC.check_covariances(_engine, n, gather_mode)


@pytest.mark.parametrize("kind", ["radius", "statistical"])
def test_outlier_removal(kind):
    WC.check_outlier_removal(_engine, kind)


def test_tightened_bound_drops_pending_sibling_leaves():
    WC.check_dropped_siblings(_engine)
