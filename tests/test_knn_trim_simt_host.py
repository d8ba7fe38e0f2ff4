"""k_knn_cov's insertion chain, pre-fill and leaf-quad loop on the CPU: the product kernels compiled for the host against the SIMT emulation of tests/emul
(which aborts on a wave operation outside wave-uniform control flow), through the shared checks of tests/knn_trim_checks.py."""
import pytest

import knn_trim_checks as KC

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


RULES = list(KC.PACKET_RULES)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n", KC.CLOUD_SIZES)
def test_cloud_sizes(n, rule):
    KC.check_cloud_size(_engine, n, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("k", KC.K_VALUES)
@pytest.mark.parametrize("n", KC.K_CLOUDS)
def test_neighbour_counts(n, k, rule):
    KC.check_k(_engine, n, k, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("gather_mode", KC.GATHER_MODES)
@pytest.mark.parametrize("method,split", [("FROBENIUS", 1), ("PLANE", 0), ("PLANE", 1)])
def test_regularizations_and_gather_modes(method, split, gather_mode, rule):
    KC.check_regularization(_engine, method, split, gather_mode, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("gather_mode", KC.GATHER_MODES)
@pytest.mark.parametrize("which", ["duplicated", "tie_heavy"])
def test_ties_at_the_kth_distance(which, gather_mode, rule):
    KC.check_ties(_engine, which, gather_mode, rule)


@pytest.mark.parametrize("rule", RULES)
def test_non_finite_input_points(rule):
    KC.check_nonfinite_input(_engine, rule)


@pytest.mark.parametrize("rule", RULES)
def test_coordinates_whose_squared_distances_overflow(rule):
    KC.check_huge_coordinates(_engine, rule)


@pytest.mark.parametrize("rule", RULES)
def test_far_outliers(rule):
    KC.check_far_outliers(_engine, rule)


@pytest.mark.parametrize("qpw", [8, 16])
def test_short_packets(qpw):
    KC.check_short_packets(_engine, qpw)


def test_statistical_outlier_removal():
    KC.check_statistical_outlier_removal(_engine)
