"""k_knn_cov's insertion chain, pre-fill and leaf-quad loop on the MI355X: the shared checks of tests/knn_trim_checks.py — cloud sizes around the packet,
the window and k, every KMAX instantiation and lists with sentinel slots, FROBENIUS / PLANE (inline and staged) under the three gather modes, ties at
the k-th distance, non-finite and huge coordinates, far outliers, 8- / 16-query packets and the prefilter's statistical outlier removal — all against
the CPU oracle."""
import pytest

import knn_trim_checks as KC

pytestmark = pytest.mark.gpu


def _hip(params):
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
    KC.check_cloud_size(_hip, n, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("k", KC.K_VALUES)
@pytest.mark.parametrize("n", KC.K_CLOUDS)
def test_neighbour_counts(n, k, rule):
    KC.check_k(_hip, n, k, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("gather_mode", KC.GATHER_MODES)
@pytest.mark.parametrize("method,split", [("FROBENIUS", 1), ("PLANE", 0), ("PLANE", 1)])
def test_regularizations_and_gather_modes(method, split, gather_mode, rule):
    KC.check_regularization(_hip, method, split, gather_mode, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("gather_mode", KC.GATHER_MODES)
@pytest.mark.parametrize("which", ["duplicated", "tie_heavy"])
def test_ties_at_the_kth_distance(which, gather_mode, rule):
    KC.check_ties(_hip, which, gather_mode, rule)


@pytest.mark.parametrize("rule", RULES)
def test_non_finite_input_points(rule):
    KC.check_nonfinite_input(_hip, rule)


@pytest.mark.parametrize("rule", RULES)
def test_coordinates_whose_squared_distances_overflow(rule):
    KC.check_huge_coordinates(_hip, rule)


@pytest.mark.parametrize("rule", RULES)
def test_far_outliers(rule):
    KC.check_far_outliers(_hip, rule)


@pytest.mark.parametrize("qpw", [8, 16])
def test_short_packets(qpw):
    KC.check_short_packets(_hip, qpw)


def test_statistical_outlier_removal():
    KC.check_statistical_outlier_removal(_hip)
