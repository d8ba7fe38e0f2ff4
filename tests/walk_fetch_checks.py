"""Shared checks of the quad walks' fetch on entry (hdl_graph_slam_amd/csrc/hgs_wave_bvh.h: QuadCursor::issue_children, quad_issue / quad_park):
the load of a node's child quad is issued when the node is entered, in front of its box tests, and parked where the walk used to fetch it.  What can
go wrong is the address of a quad nobody wanted (every entered node issues one now), the slot a held value is parked in, and a pop that re-fetches
right after a discarded load — so the cases are one target per tree shape the cursor distinguishes (binary heights 2 to 10: odd heights start at
the virtual node 0, the top slot is shared from height 7, two levels share it at height 9; a size just above a power of two leaves half the tree
padding, so entered nodes have all-pad child quads), sources around the packet and tile sizes, and targets on which nodes are entered with no
wanted child.

Every result is compared with the CPU oracle through the assertions of tests/parity_checks.py as they are: correspondences bit for bit, H / b /
fitness at their tolerances.  tests/test_walk_fetch_gpu.py runs them on the MI355X, tests/test_walk_fetch_simt_host.py on the host emulation of the
same kernels.  `make_engine(params)` builds a RegistrationHIP on the library under test.  Inputs are seeded and computed once."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
import parity_checks as PC
import walk_step_checks as WC
from hdl_graph_slam_amd import synth

DBL_MAX = WC.DBL_MAX
# 3, 5, 9, ... 513 leaves of 8 points; the number of leaves rounds up to a power of two: binary heights 2, 3, ... 10
TARGET_SIZES = (17, 33, 65, 129, 257, 513, 1025, 2049, 4097)
# shorter than a packet, exactly one packet, one point more, one point past a 256-point tile
SOURCE_SIZES = (21, 64, 65, 257)
GRID_POINTS = 2049


def tree_height(n: int) -> int:
    leaves = (n + 7) // 8
    return int(np.ceil(np.log2(leaves)))


def half_extent(n: int) -> float:
    """Half the edge of the cube a random target of n points fills: small enough that every point of the source's cube has a target point
    within max_correspondence_distance (2.5 m) — at 17 points in the 8 m cube of the larger targets most queries would have none."""
    return 1.0 if n <= 33 else (2.0 if n <= 129 else WC.HALF)


@functools.lru_cache(maxsize=None)
def random_target(n: int) -> np.ndarray:
    h = half_extent(n)
    rng = np.random.default_rng(3000 + n)
    return WC._frozen(synth.to_xyzi(rng.uniform(-h, h, (n, 3)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def random_source(m: int, h: float, far_third: bool) -> np.ndarray:
    """m points in the inner part of a target's cube; with far_third every third point is moved 10 m along x, out of every target's reach."""
    rng = np.random.default_rng(4000 + m)
    xyz = rng.uniform(-0.6 * h, 0.6 * h, (m, 3)).astype(np.float32)
    if far_third:
        xyz[::3, 0] += np.float32(WC.FAR_SHIFT)
    return WC._frozen(synth.to_xyzi(xyz))


class Pairs:
    """walk_step_checks.Pairs with parameters of the caller's choosing."""

    def __init__(self, make_engine, tgt, params=None):
        p = params if params is not None else O.default_params(O.HGS_FAST_GICP)
        self.e, self.o = make_engine(p), PC.make_oracle(p)
        for r in (self.e, self.o):
            r.setInputTarget(tgt)

    def source(self, src):
        for r in (self.e, self.o):
            r.setInputSource(src)

    def close(self):
        self.e.close()


def check_pair(pairs: Pairs, m: int, h: float):
    """The four query cases of one target / source pair: unseeded (ordered walk), seeded by that call at a moved pose (unordered walk), and both
    again with every third source point out of reach (mixed waves: the seeded call takes the ordered walk; the oracle's -1 are asserted)."""
    pairs.source(random_source(m, h, False))
    PC.check_gicp_linearize(pairs.e, pairs.o, WC.T_FIRST)
    PC.check_gicp_linearize(pairs.e, pairs.o, WC.T_MOVED)
    PC.check_fitness(pairs.e, pairs.o, WC.T_FIRST, max_ranges=(DBL_MAX, 1.0))
    pairs.source(random_source(m, h, True))
    *_, corr = pairs.o.gicp_linearize(WC.T_FIRST)
    assert (np.asarray(corr)[::3] < 0).all() and (np.delete(np.asarray(corr), np.s_[::3]) >= 0).all()     # what the case is built for
    PC.check_gicp_linearize(pairs.e, pairs.o, WC.T_FIRST)
    PC.check_gicp_linearize(pairs.e, pairs.o, WC.T_MOVED)
    PC.check_fitness(pairs.e, pairs.o, WC.T_MOVED, max_ranges=(DBL_MAX, 1.0))


def check_random_target(make_engine, n: int):
    p = O.default_params(O.HGS_FAST_GICP)
    if n < p.correspondence_randomness + 1:
        p.correspondence_randomness = 10      # the covariances of a 17-point target: k + 1 points are needed (the walks under test do not depend on k)
    pairs = Pairs(make_engine, random_target(n), p)
    try:
        for m in SOURCE_SIZES:
            check_pair(pairs, m, half_extent(n))
    finally:
        pairs.close()


def check_grid_target(make_engine):
    """Ties and the keyed fallback walk: 2049 points of the 0.25 m grid, the sources grid points themselves, at the identity and moved by exactly
    half a grid step, unseeded and seeded."""
    tgt = WC.grid_target(GRID_POINTS)
    pairs = Pairs(make_engine, tgt)
    try:
        for m in SOURCE_SIZES:
            pairs.source(tgt[3::7][:m].copy())
            for shift in ([0.0, 0.0, 0.0], [0.125, 0.0, 0.0], [0.125, 0.125, 0.0], [0.0, 0.0, 0.25]):
                T = synth.pose_matrix(shift, [0.0, 0.0, 0.0])
                PC.check_gicp_linearize(pairs.e, pairs.o, T)
                PC.check_gicp_linearize(pairs.e, pairs.o, T)      # seeded by the correspondences just found
                PC.check_fitness(pairs.e, pairs.o, T, max_ranges=(DBL_MAX, 1.0))
    finally:
        pairs.close()


@functools.lru_cache(maxsize=None)
def cluster_pairs(per_cluster: int, sites: int):
    """walk_step_checks.cluster_pairs scaled: at each site two tight clusters (2 cm) of `per_cluster` points 1.5 m apart, the sites 50 m apart.
    8 * 4^l points are the leaves below one level-l node, so with clusters of that size (or twice that) a cluster's twin is a pending sibling
    at level l of the walk of a query that sits on the cluster.  The source sits on the first cluster of site 0."""
    rng = np.random.default_rng(31)
    centres = ([0.0, 0.0, 0.0], [50.0, 0.0, 0.0], [0.0, 50.0, 0.0], [50.0, 50.0, 0.0])[:sites]
    pts = []
    for site in centres:
        for off in (0.0, 1.5):
            pts.append(np.array(site) + [off, 0.0, 0.0] + rng.normal(0, 0.02, (per_cluster, 3)))
    tgt = synth.to_xyzi(np.concatenate(pts).astype(np.float32))
    src = synth.to_xyzi(rng.normal(0, 0.02, (64, 3)).astype(np.float32))
    return WC._frozen(tgt), WC._frozen(src)


# (points per cluster, sites): 1024 points, height 7, the twin cluster pends at level 2 | 4096 points, height 9, level 3 | 8192 points, height 10:
# each cluster is two of the root's four level-4 children, which share the top slot — the twin is entered by a pop that re-fetches
DROPPED_SIBLING_CASES = {"k7": (128, 4), "k9": (512, 4), "shared_slot": (4096, 1)}


def check_dropped_siblings(make_engine, case: str):
    """Nodes entered with no wanted child, where the load issued on entry is thrown away and a pop follows it: at the first (unseeded) call every
    lane's bound is max_correspondence_distance, so the group above the source's cluster finds the twin cluster 1.5 m away wanted and leaves it
    pending; the source's own cluster pulls every bound to centimetres, and the twin, entered by a pop, has no child anybody wants.  What happens
    inside the walk is not observable: the results are what is asserted."""
    per_cluster, sites = DROPPED_SIBLING_CASES[case]
    tgt, src = cluster_pairs(per_cluster, sites)
    assert tree_height(len(tgt)) == {"k7": 7, "k9": 9, "shared_slot": 10}[case]
    pairs = Pairs(make_engine, tgt)
    try:
        pairs.source(src)
        T = synth.pose_matrix([0.01, 0.0, 0.0], [0.0, 0.0, 0.0])
        *_, corr = pairs.o.gicp_linearize(T)
        assert (np.asarray(corr) >= 0).all() and (np.asarray(corr) < per_cluster).all()      # everybody's neighbour is in the source's own cluster
        PC.check_gicp_linearize(pairs.e, pairs.o, T)
        PC.check_gicp_linearize(pairs.e, pairs.o, T)
        PC.check_fitness(pairs.e, pairs.o, T, max_ranges=(DBL_MAX, 1.0))
    finally:
        pairs.close()


def check_covariances(make_engine, n: int, gather_mode: str):
    """k_knn_cov (wave_walk_quad, which fetches on entry too) on a random target of n points, the gather pass forced to the tree walk ("0"), the
    replay of the leaf log ("1") or the per-lane leaf lists ("2"), against the oracle."""
    WC.check_covariances(make_engine, n, gather_mode)


def check_fitness_ranges(make_engine, n: int):
    """k_fitness alone (NDT_OMP parameters: no covariances, every lane unseeded — the ordered walk without tracking) at both ranges."""
    pairs = Pairs(make_engine, random_target(n), O.default_params(O.HGS_NDT_OMP))
    try:
        for m in SOURCE_SIZES:
            for far in (False, True):
                pairs.source(random_source(m, half_extent(n), far))
                PC.check_fitness(pairs.e, pairs.o, WC.T_FIRST, max_ranges=(DBL_MAX, 1.0))
    finally:
        pairs.close()
