"""The quad walks' bookkeeping on the MI355X: the shared checks of tests/walk_step_checks.py — k_gicp_linearize / k_fitness on trees of heights 9 to 12
for sources around the packet and tile sizes (unseeded, seeded, seeded with lanes out of reach), a regular grid (ties), k_knn_cov under the three
gather modes, the prefilter's outlier walks, and a leaf quad whose pending siblings are dropped by a tightened bound — all against the CPU oracle."""
import pytest

import walk_step_checks as WC

pytestmark = pytest.mark.gpu


def _hip(params):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    p = L.HgsParams()
    for name, _ in L.HgsParams._fields_:
        setattr(p, name, getattr(params, name))
    return RegistrationHIP(p)


@pytest.mark.parametrize("n", WC.TARGET_SIZES)
def test_nn1_walks_on_random_targets(n):
    WC.check_random_target(_hip, n)


def test_nn1_walks_on_a_regular_grid():
    WC.check_grid_target(_hip)


@pytest.mark.parametrize("gather_mode", ["0", "1", "2"])
@pytest.mark.parametrize("n", [2049, 8193])
def test_covariances(n, gather_mode):
    WC.check_covariances(_hip, n, gather_mode)


@pytest.mark.parametrize("kind", ["radius", "statistical"])
def test_outlier_removal(kind):
    WC.check_outlier_removal(_hip, kind)


def test_tightened_bound_drops_pending_sibling_leaves():
    WC.check_dropped_siblings(_hip)
