"""Shared checks of the quad walks' wave-uniform bookkeeping (hdl_graph_slam_amd/csrc/hgs_wave_bvh.h: QuadCursor, wave_any4, visit_leaf_quad) on trees
tall enough to use it all: heights 9 to 12, i.e. one to two levels above the levels with a park slot of their own, so that a walk descends through the
shared top slot, pops onto it (the pop re-fetches the quad) and carries the slot cursor across several shared levels — tests/parity_checks.py's
check_nn1_on_small_trees stops at 1025 target points, one level on the shared slot.

Every result is compared with the CPU oracle through the assertions of tests/parity_checks.py and tests/prefilter_checks.py as they are:
correspondences bit-exact, H / b / fitness / covariances at their tolerances, the outlier filters point for point.  tests/test_walk_step_gpu.py runs
them on the MI355X, tests/test_walk_step_simt_host.py on the host emulation of the same kernels.  `make_engine(params)` builds a RegistrationHIP on the
library under test.  Inputs are seeded and computed once."""
from __future__ import annotations

import functools
import os

import numpy as np

import oracle as O
import parity_checks as PC
import prefilter_checks as PFC
from hdl_graph_slam_amd import synth

DBL_MAX = float(np.finfo(np.float64).max)
# leaves hold 8 points and their number rounds up to a power of two: 512, 1024, 2048 and 4096 leaves — tree heights 9, 10, 11, 12
TARGET_SIZES = (2049, 4097, 8193, 20011)
# shorter than a packet, exactly one packet, one point more, a partial second packet, one point past a 256-point tile
SOURCE_SIZES = (21, 64, 65, 150, 257)
GRID_STEP = 0.25
HALF = 4.0          # the random targets fill the cube [-HALF, HALF]^3
FAR_SHIFT = 10.0    # a source point moved this far along x leaves the cube by more than max_correspondence_distance (2.5 m)


def _frozen(cloud: np.ndarray) -> np.ndarray:
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def random_target(n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    return _frozen(synth.to_xyzi(rng.uniform(-HALF, HALF, (n, 3)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def grid_target(n: int = 8193) -> np.ndarray:
    """n points of a regular 0.25 m grid (32 x 32 x 9 nodes, shuffled): every coordinate and every half-step shift is exact in float."""
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(9), indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(7)
    pts = (g[rng.permutation(len(g))[:n]] * GRID_STEP - [4.0, 4.0, 1.0]).astype(np.float32)
    return _frozen(synth.to_xyzi(pts))


@functools.lru_cache(maxsize=None)
def random_source(m: int, far_third: bool) -> np.ndarray:
    """m points well inside the targets' cube; with far_third every third point is moved 10 m along x: no target point within 2.5 m of it at
    any of the poses below, in the same packets as points that do have one."""
    rng = np.random.default_rng(2000 + m)
    xyz = rng.uniform(-HALF + 1.5, HALF - 1.5, (m, 3)).astype(np.float32)
    if far_third:
        xyz[::3, 0] += np.float32(FAR_SHIFT)
    return _frozen(synth.to_xyzi(xyz))


T_FIRST = synth.pose_matrix([0.05, -0.02, 0.01], [0.0, 0.0, 0.01])
T_MOVED = synth.pose_matrix([0.06, -0.02, 0.01], [0.0, 0.0, 0.012])


class Pairs:
    """One engine and one oracle holding a target (index and covariances built once); the sources come and go."""

    def __init__(self, make_engine, tgt):
        p = O.default_params(O.HGS_FAST_GICP)
        self.e, self.o = make_engine(p), PC.make_oracle(p)
        for r in (self.e, self.o):
            r.setInputTarget(tgt)

    def source(self, src):
        for r in (self.e, self.o):
            r.setInputSource(src)

    def close(self):
        self.e.close()


def check_pair(pairs: Pairs, m: int):
    """The 1-NN walks of k_gicp_linearize and k_fitness for one source size: unseeded (ordered walk), seeded by that call at a slightly moved pose
    (unordered walk), and the same two calls with a third of the source out of reach (lanes without a correspondence carry no seed: the seeded
    call's waves hold seeded and unseeded lanes and take the ordered walk)."""
    pairs.source(random_source(m, False))
    PC.check_gicp_linearize(pairs.e, pairs.o, T_FIRST)
    PC.check_gicp_linearize(pairs.e, pairs.o, T_MOVED)
    PC.check_fitness(pairs.e, pairs.o, T_FIRST, max_ranges=(DBL_MAX, 1.0))
    src = random_source(m, True)
    pairs.source(src)
    *_, corr = pairs.o.gicp_linearize(T_FIRST)
    assert (np.asarray(corr)[::3] < 0).all() and (np.delete(np.asarray(corr), np.s_[::3]) >= 0).all()     # what the case is built for
    PC.check_gicp_linearize(pairs.e, pairs.o, T_FIRST)
    PC.check_gicp_linearize(pairs.e, pairs.o, T_MOVED)
    PC.check_fitness(pairs.e, pairs.o, T_MOVED, max_ranges=(DBL_MAX, 1.0))


def check_random_target(make_engine, n: int):
    pairs = Pairs(make_engine, random_target(n))
    try:
        for m in SOURCE_SIZES:
            check_pair(pairs, m)
    finally:
        pairs.close()


def check_grid_target(make_engine):
    """Ties: the sources are grid points themselves, at the identity (distance 0) and moved by exactly half a grid step (two, four equidistant grid
    points, in different leaves for most queries: the tie fallback to the keyed walk), unseeded and seeded."""
    tgt = grid_target()
    pairs = Pairs(make_engine, tgt)
    try:
        for m in SOURCE_SIZES:
            pairs.source(tgt[5::31][:m].copy())
            for shift in ([0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.125, 0.125, 0.0], [0.0, 0.0, 0.25]):
                T = synth.pose_matrix(shift, [0.0, 0.0, 0.0])
                PC.check_gicp_linearize(pairs.e, pairs.o, T)
                PC.check_gicp_linearize(pairs.e, pairs.o, T)      # seeded by the correspondences just found
                PC.check_fitness(pairs.e, pairs.o, T, max_ranges=(DBL_MAX, 1.0))
    finally:
        pairs.close()


def check_covariances(make_engine, n: int, gather_mode: str):
    """k_knn_cov (wave_walk_quad with the k-NN radius and gather lanes) with the gather pass forced to the tree walk, the replay of the leaf log, or
    chosen by launch shape (engine option knn_replay, applied when the engine is created)."""
    old = os.environ.get("HGS_ENGINE_OPTIONS")
    os.environ["HGS_ENGINE_OPTIONS"] = "knn_replay=" + gather_mode
    try:
        e = make_engine(O.default_params(O.HGS_FAST_GICP))
        cloud = random_target(n)
        e.setInputTarget(cloud)
        PC.check_covariances(e, cloud, 20)
        e.close()
    finally:
        if old is None:
            os.environ.pop("HGS_ENGINE_OPTIONS", None)
        else:
            os.environ["HGS_ENGINE_OPTIONS"] = old


def check_outlier_removal(make_engine, kind: str):
    """The prefilter's outlier walks (wave_walk_quad with the radius-count and k-NN distance lanes) on a 4097-point cloud, against the oracle."""
    cloud = PFC.mixture(4097, 3)
    fields = PFC._radius(2.5, 2) if kind == "radius" else PFC._stat()
    reg = make_engine(O.default_params(O.HGS_FAST_GICP))
    try:
        got = PFC.expect_oracle(reg, cloud, fields, kind)
        assert 0 < len(got) < len(cloud), kind      # the filter removes something and keeps something
    finally:
        reg.close()


@functools.lru_cache(maxsize=None)
def cluster_pairs():
    """Four sites 50 m apart, at each two tight clusters (2 cm) of 16 points 1.5 m apart: in Hilbert order a site is 32 consecutive points = one
    leaf quad, two leaves per cluster.  The source sits on the first cluster of site 0."""
    rng = np.random.default_rng(21)
    pts = []
    for site in ([0.0, 0.0, 0.0], [50.0, 0.0, 0.0], [0.0, 50.0, 0.0], [50.0, 50.0, 0.0]):
        for off in (0.0, 1.5):
            pts.append(np.array(site) + [off, 0.0, 0.0] + rng.normal(0, 0.02, (16, 3)))
    tgt = synth.to_xyzi(np.concatenate(pts).astype(np.float32))
    src = synth.to_xyzi(rng.normal(0, 0.02, (64, 3)).astype(np.float32))
    return _frozen(tgt), _frozen(src)


def check_dropped_siblings(make_engine):
    """A tightened bound drops a pending sibling leaf: at the first (unseeded) call every lane's bound is max_correspondence_distance, so the leaf
    parent of site 0 finds all four leaves wanted; the first visit — the source's own cluster — pulls every lane's bound to centimetres and the two
    leaves of the cluster 1.5 m away are dropped by the re-test.  The drop is internal: the results are what is asserted."""
    tgt, src = cluster_pairs()
    pairs = Pairs(make_engine, tgt)
    try:
        pairs.source(src)
        T = synth.pose_matrix([0.01, 0.0, 0.0], [0.0, 0.0, 0.0])
        *_, corr = pairs.o.gicp_linearize(T)
        assert (np.asarray(corr) >= 0).all() and (np.asarray(corr) < 16).all()      # everybody's neighbour is in the source's own cluster
        PC.check_gicp_linearize(pairs.e, pairs.o, T)
        PC.check_gicp_linearize(pairs.e, pairs.o, T)
        PC.check_fitness(pairs.e, pairs.o, T, max_ranges=(DBL_MAX, 1.0))
    finally:
        pairs.close()
