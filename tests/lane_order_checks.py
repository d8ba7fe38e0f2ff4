"""Shared checks of the ordered lanes of a FAST_GICP batch (hdl_graph_slam_amd/csrc/hgs_engine.hip: lane_order_of, plan_lanes, open_lanes; option
"lane_order"): a batch of 8 or more problems that opens several lanes is run in an order of its own — farthest guess first, the first half on
highest-priority streams — and handed back in the caller's order.  The yardstick is exact: a record depends on its own target, source and guess only,
so every record with lane_order = 1 equals, bit for bit, the record with lane_order = 0 and the record of the problem run alone.  What can go wrong is
the way back (records, best_candidate, the sharded path's slots), the plan (who gets ordered lanes, how many streams), and the hint's corner cases
(ties, equal hints, non-finite guesses).

tests/test_lane_order_gpu.py runs them on the MI355X, tests/test_lane_order_simt_host.py on the host emulation of the same kernels.  The clouds have
2-3 k points; "batch_lanes" = 4 makes batches of that size take the multi-lane path.  Inputs are seeded and computed once."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from hdl_graph_slam_amd import _lib as L, synth, workloads
from hdl_graph_slam_amd.registration import HgsError, RegistrationHIP

N = 13
MAX_RANGE = 4.0
BATCH_SIZES = (1, 2, 3, 5, 8, 9, 13)
MIN_ORDERED = 8          # kLaneOrderMinProblems
FIELDS = [f for f in L.RESULT_DTYPE.names if f != "candidate_id"]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def scene():
    """One query keyframe and 13 candidates cut from 4 ray-cast VLP-16 scans within 3 m of it (voxel 0.5 m: 1800-2300 points each); the guesses'
    translation norms are distinct and lie between 0.3 and 3.5 m."""
    wl = workloads.make_loop_closure_set("VLP-16", 3, n_candidates=N, n_distinct=4, downsample=0.5, spread=3.0, guess_noise=(0.2, 1.0))
    assert all(1500 < len(c) < 3000 for c in wl.candidates + [wl.target])
    for a in wl.candidates + [wl.target] + wl.guesses:
        _frozen(a)
    return wl


def hint(g) -> np.float32:
    """The engine's hint of a guess (row-major 4x4 here): squared translation norm in float, FLT_MAX if that is not finite."""
    t = np.asarray(g, np.float32)[:3, 3]
    with np.errstate(all="ignore"):
        d2 = np.float32(np.float32(t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return d2 if np.isfinite(d2) else np.finfo(np.float32).max


def run_order(guesses):
    """Caller positions in the order the engine runs them: stable, hint descending."""
    h = np.array([hint(g) for g in guesses], np.float64)
    return list(np.argsort(-h, kind="stable"))


def guesses_of(variant: str):
    g = [np.array(x, np.float32) for x in scene().guesses]
    if variant == "same":          # one translation for all: every hint equal, the stable order is the caller's
        for x in g:
            x[:3, 3] = g[0][:3, 3]
        assert run_order(g) == list(range(N))
    elif variant == "ties":        # pairs of exactly tied hints (the same translation, and its mirror image), in different halves of the caller's list
        for i in range(N // 2):
            g[N - 1 - i][:3, 3] = g[i][:3, 3] * np.float32(-1 if i % 2 else 1)
        assert len({float(hint(x)) for x in g}) == N - N // 2
    elif variant == "nonfinite":   # a NaN and an infinite translation: both sort to the front, the NaN (caller position 2) first
        g[2][0, 3] = np.nan
        g[7][1, 3] = np.inf
        assert run_order(g)[:2] == [2, 7]
    else:
        assert variant == "distinct" and len({float(hint(x)) for x in g}) == N
    return g


def make_engine():
    e = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
    e.set_option("batch_lanes", 4)
    return e


class Case:
    """One FAST_GICP engine ("batch_lanes" = 4) with the scene's target set and its candidates resident."""

    def __init__(self, engine_factory=make_engine):
        self.factory = engine_factory
        self.e = engine_factory()
        wl = scene()
        self.target = self.e.upload(wl.target)
        self.e.setInputTarget(self.target)
        self.clouds = [self.e.upload(c) for c in wl.candidates]
        self._alone = None

    def batch(self, idx, guesses, lane_order, clouds=None):
        """(records, best, (lanes, ahead lanes)) of one hgs_loop_match_batch over the candidates idx."""
        self.e.set_option("lane_order", lane_order)
        rec, best = self.e.loop_match_batch([(clouds or self.clouds)[i] for i in idx], [guesses[i] for i in idx], MAX_RANGE)
        return rec, best, self.e.lane_plan()[:2]

    def alone(self):
        """Every candidate registered alone from its guess (lane_order = 0), once."""
        if self._alone is None:
            g = guesses_of("distinct")
            self._alone = [self.batch([i], g, 0)[0][0].copy() for i in range(N)]
        return self._alone

    def close(self):
        for c in self.clouds + [self.target]:
            c.close()
        self.e.close()


def assert_same_records(rec, ref, where):
    assert len(rec) == len(ref), where
    for i in range(len(rec)):
        for f in FIELDS:
            assert np.asarray(rec[i][f]).tobytes() == np.asarray(ref[i][f]).tobytes(), (where, i, f, rec[i][f], ref[i][f])


def expected_plan(B, lane_order):
    lanes = min(4, B)
    return (lanes, (2 if lanes >= 4 else 1) if lane_order and B >= MIN_ORDERED and lanes > 1 else 0)


def check_batch_size(case: Case, B: int):
    """The first B candidates: ordered against contiguous lanes and against every problem alone; the lane plan is the ordered one from 8 problems up."""
    g = guesses_of("distinct")
    idx = list(range(B))
    rec0, best0, plan0 = case.batch(idx, g, 0)
    rec1, best1, plan1 = case.batch(idx, g, 1)
    assert plan0 == expected_plan(B, 0) and plan1 == expected_plan(B, 1), (B, plan0, plan1)
    assert rec1.tobytes() == rec0.tobytes() and best1 == best0, B
    assert list(rec1["candidate_id"]) == idx
    assert_same_records(rec1, case.alone()[:B], ("alone", B))
    assert rec1["converged"].all() and (rec1["iterations"] >= 2).all()        # the check is about something: every problem iterates and converges,
    assert B < 8 or len(set(rec1["iterations"])) > 1                          # ... not all in the same number of rounds


def check_guess_variant(case: Case, variant: str, B: int):
    g = guesses_of(variant)
    idx = list(range(B))
    rec0, best0, _ = case.batch(idx, g, 0)
    rec1, best1, plan1 = case.batch(idx, g, 1)
    assert plan1 == expected_plan(B, 1)
    assert case.e.batch_order() == run_order(g[:B])              # the engine's order is the model's: ties keep the caller's order, NaN and inf lead
    assert rec1.tobytes() == rec0.tobytes() and best1 == best0, (variant, B)
    assert list(rec1["candidate_id"]) == idx


def check_repeated_sources(case: Case):
    """One cloud object twice in a batch is refused as before; the same POINTS in several clouds of a batch, and the target cloud itself as a candidate,
    give what contiguous lanes give."""
    g = guesses_of("distinct")
    for lane_order in (0, 1):
        case.e.set_option("lane_order", lane_order)
        with pytest.raises(HgsError, match="distinct"):
            case.e.loop_match_batch([case.clouds[i] for i in (0, 1, 2, 3, 4, 5, 6, 0)], [g[i] for i in range(8)], MAX_RANGE)
    wl = scene()
    src = [0, 1, 0, 2, 1, 3, 0]                       # scan 0 three times, scan 1 twice
    extra = [case.e.upload(wl.candidates[i]) for i in src] + [case.target]
    gs = [g[i] for i in src] + [synth.pose_matrix([0.2, -0.1, 0.0], [0.0, 0.0, 0.02]).astype(np.float32)]
    try:
        idx = list(range(len(extra)))
        rec0, best0, _ = case.batch(idx, gs, 0, clouds=extra)
        rec1, best1, plan1 = case.batch(idx, gs, 1, clouds=extra)
        assert plan1 == (4, 2)
        assert rec1.tobytes() == rec0.tobytes() and best1 == best0
        assert_same_records(rec1[[0, 2, 6]], [rec1[0]] * 3, "the same points from the same guess")
        assert rec1["converged"][7] and rec1["fitness_score"][7] < 1e-6      # the target against itself
    finally:
        for c in extra[:-1]:
            c.close()


def check_tie_rule(case: Case):
    """Two problems with equal (and best) scores whose run positions the ordering puts into different groups: best_candidate is the later one in the
    CALLER's order (loop_detector.hpp:146-153 replaces on an equal score), as with contiguous lanes."""
    wl = scene()
    g = guesses_of("distinct")
    twin_guess = synth.pose_matrix([0.3, 0.0, 0.0], [0.0, 0.0, 0.01]).astype(np.float32)
    near_guess = synth.pose_matrix([0.1, 0.0, 0.0], [0.0, 0.0, 0.0]).astype(np.float32)
    near = [case.e.upload(synth.transform_cloud(wl.candidates[k], wl.T_gt[k])) for k in (0, 2, 8)]    # candidates moved into the query's frame
    twin = case.e.upload(wl.target)
    far = (3, 5, 11)                                                                                   # guesses 2.6, 2.0 and 3.5 m out
    #          caller position: 0      1            2                 3        4                 5        6     7
    clouds = [near[0], case.target, case.clouds[far[0]], near[1], case.clouds[far[1]], near[2], twin, case.clouds[far[2]]]
    gs = [near_guess, twin_guess, g[far[0]], near_guess, g[far[1]], near_guess, twin_guess, g[far[2]]]
    try:
        idx = list(range(8))
        rec0, best0, _ = case.batch(idx, gs, 0, clouds=clouds)
        assert case.e.batch_order() == []
        rec1, best1, plan1 = case.batch(idx, gs, 1, clouds=clouds)
        assert plan1 == (4, 2)
        order = case.e.batch_order()                                # the order the ENGINE ran in
        assert order == run_order(gs)
        assert order.index(1) == 3 and order.index(6) == 4          # the last of the ahead group (4 of 8) and the first of the other
        assert rec1.tobytes() == rec0.tobytes()
        assert_same_records(rec1[[1]], rec1[[6]], "twins")
        others = [i for i in idx if i not in (1, 6)]
        assert rec1["converged"][[1, 6]].all() and rec1["fitness_score"][1] < rec1["fitness_score"][others].min()
        assert best1 == best0 == 6
    finally:
        for c in near + [twin]:
            c.close()


def check_sharded_world_one(case: Case):
    """hgs_loop_match_batch_sharded at world size 1, the rank listing its candidates in an order of its own: slots and candidate ids in caller order."""
    g = guesses_of("distinct")
    rec, best, _ = case.batch(list(range(9)), g, 0)
    case.e.comm_init(0, 1, RegistrationHIP.comm_unique_id())
    try:
        listed = [3, 0, 8, 4, 1, 7, 2, 6, 5]
        for lane_order in (0, 1):
            case.e.set_option("lane_order", lane_order)
            rec_s, best_s = case.e.loop_match_batch_sharded([case.clouds[i] for i in listed], listed, [g[i] for i in listed], 9, MAX_RANGE)
            assert case.e.lane_plan()[:2] == expected_plan(9, lane_order)
            assert list(rec_s["candidate_id"]) == list(range(9)) and best_s == best
            assert_same_records(rec_s, rec, ("sharded", lane_order))
    finally:
        case.e.comm_finalize()


def check_sharded_two_ranks(run_ranks, engine_factory=make_engine):
    """Two ranks of 9 and 8 candidates (17 in total, interleaved ids), both with ordered lanes: every rank receives all records in candidate order,
    bitwise those of one unsharded batch with contiguous lanes.  run_ranks(world, body) drives body(rank, unique_id) per rank."""
    wl = scene()
    n_total, world = 17, 2
    base = guesses_of("distinct")
    guesses = [base[i % N].copy() for i in range(n_total)]
    for i in range(N, n_total):
        guesses[i][:3, 3] *= np.float32(0.5)          # (candidates 13..16 are scans 0..3 again from a guess of their own)
    shards = [list(range(0, n_total, 2)), list(range(1, n_total, 2))]

    def body(rank, uid):
        reg = engine_factory()
        reg.set_option("lane_order", 1)
        reg.setInputTarget(wl.target)
        reg.comm_init(rank, world, uid)
        mine = shards[rank][::-1]                     # listed backwards
        rec, best = reg.loop_match_batch_sharded([reg.upload(wl.candidates[i % N]) for i in mine], mine, [guesses[i] for i in mine], n_total, MAX_RANGE)
        plan = reg.lane_plan()[:2]
        reg.close()
        return rec, best, plan
    res = run_ranks(world, body)
    one = engine_factory()
    one.set_option("lane_order", 0)
    one.setInputTarget(wl.target)
    rec, best = one.loop_match_batch([one.upload(wl.candidates[i % N]) for i in range(n_total)], guesses, MAX_RANGE)
    one.close()
    for rank, (rec_r, best_r, plan) in enumerate(res):
        assert plan == (4, 2), (rank, plan)
        assert list(rec_r["candidate_id"]) == list(range(n_total)) and best_r == best
        assert_same_records(rec_r, rec, ("rank", rank))


def check_fitness_after_batch(case: Case):
    """hgs_fitness right after a batch, on a source that was one of its candidates (its correspondence seeds are the batch's): a candidate of the ahead
    group and one of the other group, each against the same call behind contiguous lanes and against its own record."""
    g = guesses_of("distinct")
    idx = list(range(9))
    order = run_order([g[i] for i in idx])
    for k in (order[0], order[-1]):
        case.e.setInputSource(case.clouds[k])
        got = []
        for lane_order in (0, 1):
            rec, _, plan = case.batch(idx, g, lane_order)
            assert plan == expected_plan(len(idx), lane_order)
            T = np.array(rec[k]["final_transformation"], np.float32).reshape(4, 4).T
            got.append((case.e.getFitnessScore(MAX_RANGE, T=T), case.e.last_num_inliers, float(rec[k]["fitness_score"]), int(rec[k]["num_inliers"])))
        assert got[0] == got[1], (k, got)
        # the record's own score: the same exact 1-NN distances at the same pose, summed in double in the same or another grouping
        assert got[1][1] == got[1][3] and np.isclose(got[1][0], got[1][2], rtol=1e-12, atol=0.0), (k, got)


def check_profiling_keeps_one_lane(case: Case):
    """Under profiling a batch runs on one lane and is not ordered."""
    g = guesses_of("distinct")
    idx = list(range(9))
    rec0, best0, _ = case.batch(idx, g, 0)
    case.e.profile_enable(True)
    try:
        rec1, best1, plan1 = case.batch(idx, g, 1)
    finally:
        case.e.profile_read()
        case.e.profile_enable(False)
    assert plan1 == (1, 0)
    assert rec1.tobytes() == rec0.tobytes() and best1 == best0


@functools.lru_cache(maxsize=None)
def big_scene():
    """8 candidates above 96 tiles of 256 points (raw VLP-16 scans), the size from which a batch opens four lanes by itself ("batch_lanes" = 0)."""
    wl = workloads.make_loop_closure_set("VLP-16", 3, n_candidates=8, n_distinct=2, spread=3.0, guess_noise=(0.2, 1.0))
    assert all(len(c) > 96 * 256 for c in wl.candidates)
    return wl


def check_queue_budget():
    """The hardware-queue budget at 4 (GPU_MAX_HW_QUEUES) in a process whose streams are known — run in a process of its own
    (run_queue_budget_in_child), where nothing but this function's engines exists.  A second engine is alive throughout.
      1. a fresh engine: two streams are held, two are free; the ordered batch opens three lanes, one of them ahead — exactly two new streams (one
         priority stream, one plain), none beyond the budget — and returns what contiguous lanes return;
      2. an engine that already owns plain lane streams and finds the budget spent: no room for a priority stream, the plain plan stands with the
         lanes it owns, no stream is added, same records."""
    assert (int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) or 4) == 4
    wl = big_scene()

    def engine(lane_order):
        e = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))      # "batch_lanes" = 0: the budget applies
        e.set_option("lane_order", lane_order)
        e.setInputTarget(wl.target)
        return e, [e.upload(c) for c in wl.candidates]
    ref, clouds = engine(0)
    assert ref.lane_plan()[2] == 1
    rec0, best0 = ref.loop_match_batch(clouds, wl.guesses, MAX_RANGE)
    assert ref.lane_plan() == (4, 0, 4)          # alone in the process: four contiguous lanes
    ref.close()
    other, _ = engine(0)
    try:
        # 1.
        e, clouds = engine(1)
        assert e.lane_plan()[2] == 2
        rec1, best1 = e.loop_match_batch(clouds, wl.guesses, MAX_RANGE)
        assert e.lane_plan() == (3, 1, 4), e.lane_plan()
        assert e.batch_order() == run_order(wl.guesses)
        assert rec1.tobytes() == rec0.tobytes() and best1 == best0
        e.close()
        assert other.lane_plan()[2] == 1
        # 2.
        e, clouds = engine(0)
        rec2, best2 = e.loop_match_batch(clouds, wl.guesses, MAX_RANGE)
        assert e.lane_plan() == (3, 0, 4), e.lane_plan()      # its own stream and two plain lane streams: the budget is spent
        e.set_option("lane_order", 1)
        rec3, best3 = e.loop_match_batch(clouds, wl.guesses, MAX_RANGE)
        assert e.lane_plan() == (3, 0, 4), e.lane_plan()
        assert e.batch_order() == []
        assert rec2.tobytes() == rec0.tobytes() and rec3.tobytes() == rec0.tobytes() and best2 == best3 == best0
        e.close()
    finally:
        other.close()


def run_queue_budget_in_child(lib_path=None):
    """check_queue_budget in a fresh interpreter with GPU_MAX_HW_QUEUES=4 (the library reads the budget once per process, and the count of streams is
    per process): the test is about a process's streams."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GPU_MAX_HW_QUEUES="4", PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests"), os.environ.get("PYTHONPATH", "")]))
    env.pop("HGS_ENGINE_OPTIONS", None)
    code = "import lane_order_checks as LC\n"
    if lib_path:
        code += f"LC.L.LIB_PATH, LC.L._lib = {lib_path!r}, None\n"
    code += "LC.check_queue_budget()\nprint('BUDGET_OK')\n"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "BUDGET_OK" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])


BIG_TILES = 100      # tiles of 256 points per problem above which a FAST_GICP batch opens four lanes by itself


def check_plan_arithmetic(engine_factory=make_engine):
    """plan_lanes (host code) through hgs_debug_plan_lanes: the plan of a batch of 8 large problems against an assumed number of streams held by the
    process (budget 4 unless GPU_MAX_HW_QUEUES says otherwise), for an engine that owns nothing, one that owns priority streams, and one that owns
    plain lane streams.  Nothing runs but the two small batches that make an engine own its streams."""
    budget = int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) or 4
    g = guesses_of("distinct")

    def fresh():
        e = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
        return e
    e = fresh()
    try:
        # nothing owned: needs one new stream per lane beyond its own; the largest ordered plan that fits
        for held, want in ((budget - 3, (4, 2)), (budget - 2, (3, 1)), (budget - 1, (2, 1)), (budget, (1, 0)), (budget + 5, (1, 0))):
            assert e.plan_lanes(8, BIG_TILES, True, held) == want, (held, want, e.plan_lanes(8, BIG_TILES, True, held))
            assert e.plan_lanes(8, BIG_TILES, False, held) == (want[0], 0)
        assert e.plan_lanes(7, BIG_TILES, True, budget - 3) == (4, 0)          # fewer than 8 problems: never ordered
        assert e.plan_lanes(64, 9, True, budget - 3) == (1, 0)                 # small problems, 576 tiles in all: one lane, never ordered
        assert e.plan_lanes(64, 480, True, budget - 3) == (4, 2)               # the benchmark's batch
        e.set_option("lane_order", 0)
        assert e.plan_lanes(8, BIG_TILES, True, budget - 3) == (4, 0)
        e.set_option("lane_order", 1)
        e.profile_enable(True)
        assert e.plan_lanes(8, BIG_TILES, True, budget - 3) == (1, 0)          # profiling: one lane
        e.profile_enable(False)
    finally:
        e.close()
    for first_order, owned_plan in ((1, (4, 2)), (0, (4, 0))):
        c = Case(engine_factory)                 # "batch_lanes" = 4: the small batch below opens four lanes whatever the budget says
        try:
            _, _, plan = c.batch(list(range(8)), g, first_order)
            assert plan == owned_plan
            c.e.set_option("batch_lanes", 0)
            c.e.set_option("lane_order", 1)
            if first_order:      # owns two priority streams and one lane stream: the ordered plan costs nothing new, the plain one two streams
                assert c.e.plan_lanes(8, BIG_TILES, True, budget) == (4, 2)
                assert c.e.plan_lanes(8, BIG_TILES, False, budget) == (2, 0)
                assert c.e.plan_lanes(8, BIG_TILES, False, budget - 2) == (4, 0)
            else:                # owns three plain lane streams: no room for a priority stream, the plain plan stands; with room for two, ordered
                assert c.e.plan_lanes(8, BIG_TILES, True, budget) == (4, 0)
                assert c.e.plan_lanes(8, BIG_TILES, True, budget - 1) == (4, 0)
                assert c.e.plan_lanes(8, BIG_TILES, True, budget - 2) == (4, 2)
        finally:
            c.close()
