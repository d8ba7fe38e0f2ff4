"""Ordered lanes of a FAST_GICP batch on the CPU: the engine's host code (the hint, the order, the lane plan, the way back to the caller's order) and
the product kernels compiled for the host against the SIMT emulation of tests/emul, through the shared checks of tests/lane_order_checks.py.  The
emulated runtime has no stream priorities (the engine's priority streams are plain streams there): what is checked is everything but the
scheduling — and two ranks of the sharded entry point, which one GPU test process cannot host.  The hardware-queue budget with real batches is checked on the
device only (without "batch_lanes" a batch opens several lanes from 25 k points per problem up, minutes of emulation); its arithmetic is checked here
through the plan read-out."""
import threading

import pytest

import lane_order_checks as LC

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


def _run_ranks(world, body):
    """body(rank, unique_id) per rank on a host thread of its own (the emulated communicator stands in for RCCL)."""
    from hdl_graph_slam_amd.registration import RegistrationHIP
    uid = RegistrationHIP.comm_unique_id()
    out, errs = [None] * world, []

    def run(rank):
        try:
            out[rank] = body(rank, uid)
        except Exception as exc:  # noqa: BLE001
            errs.append((rank, repr(exc)))
    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not any(t.is_alive() for t in threads), "a rank is still blocked in the collective"
    assert not errs, errs
    return out


def test_sharded_entry_point_two_ranks():
    LC.check_sharded_two_ranks(_run_ranks)


def test_fitness_right_after_an_ordered_batch(case):
    LC.check_fitness_after_batch(case)


def test_profiling_keeps_one_lane(case):
    LC.check_profiling_keeps_one_lane(case)


def test_lane_plan_arithmetic():
    LC.check_plan_arithmetic()
