"""The quad walks' fetch on entry on the CPU: the product kernels compiled for the host against the SIMT emulation of tests/emul (which aborts on a
wave operation outside wave-uniform control flow), through the shared checks of tests/walk_fetch_checks.py."""
import pytest

import walk_fetch_checks as FC

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


@pytest.mark.parametrize("n", FC.TARGET_SIZES)
def test_nn1_walks_on_every_tree_shape(n):
    FC.check_random_target(_engine, n)


def test_nn1_walks_on_a_regular_grid():
    FC.check_grid_target(_engine)


@pytest.mark.parametrize("case", sorted(FC.DROPPED_SIBLING_CASES))
def test_pending_siblings_entered_with_no_wanted_child(case):
    FC.check_dropped_siblings(_engine, case)


@pytest.mark.parametrize("n", [1025, 4097])     # binary heights 7 (the first shared top slot) and 9 (two shared levels)
def test_fitness_at_both_ranges(n):
    FC.check_fitness_ranges(_engine, n)


@pytest.mark.parametrize("gather_mode", ["0", "1", "2"])
@pytest.mark.parametrize("n", [513, 2049])
def test_covariances(n, gather_mode):
    FC.check_covariances(_engine, n, gather_mode)
