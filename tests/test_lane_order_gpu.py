"""Ordered lanes of a FAST_GICP batch on the MI355X: the shared checks of tests/lane_order_checks.py — records with "lane_order" = 1 against
"lane_order" = 0 and against every problem alone, bit for bit, for batches below and above the threshold; guesses at distinct, equal, tied and
non-finite distances; repeated points and the target as a candidate; best_candidate's tie rule across the two groups; the sharded entry point at
world size 1; hgs_fitness behind a batch; the lane plan under profiling; the hardware-queue budget with a second engine alive."""
import pytest

import lane_order_checks as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    c = LC.Case()
    yield c
    c.close()


@pytest.mark.parametrize("B", LC.BATCH_SIZES)
def test_records_equal_contiguous_lanes_and_every_problem_alone(case, B):
    LC.check_batch_size(case, B)


@pytest.mark.parametrize("variant,B", [("same", 13), ("ties", 13), ("ties", 8), ("nonfinite", 9)])
def test_guesses_at_equal_tied_and_non_finite_distances(case, variant, B):
    LC.check_guess_variant(case, variant, B)


def test_repeated_points_and_the_target_as_a_candidate(case):
    LC.check_repeated_sources(case)


def test_best_candidate_of_equal_scores_in_different_groups(case):
    LC.check_tie_rule(case)


def test_sharded_entry_point_world_one(case):
    LC.check_sharded_world_one(case)


def test_fitness_right_after_an_ordered_batch(case):
    LC.check_fitness_after_batch(case)


def test_profiling_keeps_one_lane(case):
    LC.check_profiling_keeps_one_lane(case)


def test_priority_streams_count_against_the_queue_budget():
    LC.run_queue_budget_in_child()


def test_lane_plan_arithmetic():
    LC.check_plan_arithmetic()
