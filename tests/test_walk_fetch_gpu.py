"""The quad walks' fetch on entry on the MI355X: the shared checks of tests/walk_fetch_checks.py — k_gicp_linearize / k_fitness on one target per
tree shape (binary heights 2 to 10) for sources around the packet and tile sizes (unseeded, seeded, both with lanes out of reach), a regular grid
(ties), targets whose pending siblings are entered with no wanted child (also where the pop re-fetches), k_fitness at both ranges — all against
the CPU oracle."""
import pytest

import walk_fetch_checks as FC

pytestmark = pytest.mark.gpu


def _hip(params):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    p = L.HgsParams()
    for name, _ in L.HgsParams._fields_:
        setattr(p, name, getattr(params, name))
    return RegistrationHIP(p)


@pytest.mark.parametrize("n", FC.TARGET_SIZES)
def test_nn1_walks_on_every_tree_shape(n):
    FC.check_random_target(_hip, n)


def test_nn1_walks_on_a_regular_grid():
    FC.check_grid_target(_hip)


@pytest.mark.parametrize("case", sorted(FC.DROPPED_SIBLING_CASES))
def test_pending_siblings_entered_with_no_wanted_child(case):
    FC.check_dropped_siblings(_hip, case)


@pytest.mark.parametrize("n", [1025, 4097])     # binary heights 7 (the first shared top slot) and 9 (two shared levels)
def test_fitness_at_both_ranges(n):
    FC.check_fitness_ranges(_hip, n)


@pytest.mark.parametrize("gather_mode", ["0", "1", "2"])
@pytest.mark.parametrize("n", [513, 2049])
def test_covariances(n, gather_mode):
    FC.check_covariances(_hip, n, gather_mode)
