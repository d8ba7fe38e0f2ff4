"""Shared checks of k_knn_cov's insertion chain, pre-fill loop and leaf-quad loop (hdl_graph_slam_amd/csrc/hgs_wave_bvh.h: KnnRadiusLane::insert /
visit_leaf, wave_walk_quad; hgs_kernels.hip: k_knn_cov, k_cov_regularize, problem_cloud) at the smallest inputs where each of them can go wrong:

  * the chain takes every lane's distance as it is (no select in front of it): a lane that does not accept a candidate — a distance equal to its k-th, a
    +inf distance to a pad point or from overflow, an idle lane's all -1 list, a list whose low slots hold the -1 sentinel (k < KMAX) — must keep its list;
  * the pre-fill takes two window points per iteration and a single one at an odd count;
  * the walk's skip window, leaf number and parked record address are scalars;
  * the cloud's arrays are reached through global pointers.

Every covariance is compared with the CPU oracle through tests/parity_checks.py's check_covariances as it is (relative 5e-6 per point: float storage
and summation order; a neighbour set that differs by one point moves a covariance by orders of magnitude more), the statistical outlier removal — the
same lane type under the generic walk — point for point through tests/prefilter_checks.py.

Which kernel a case launches is decided by the engine (hgs_engine.hip, queries_per_wave; hgs_kernels.hip, launch_knn_cov_t), so every check takes the packet
rule as a parameter (PACKET_RULES) and runs under both:
  * "32": engine option knn_qpw_tiny=0 — 32-query packets, the k_knn_cov<KMAX, REG, GATHER, false> instantiations (KMAX 8 / 16 / 20 / 32 / 64 by k), the ones
    the flagship batch runs (there with 64-query packets: a launch of >= 600 000 queries, far beyond a quick test; the packet size is a run-time argument of the
    same code).  The pre-fill window is the packet itself: a packet of w points runs w / 2 pair iterations and a tail iteration when w is odd.
  * "tiered": the engine's default (knn_qpw_tiny=-1) — every launch here is below 32768 queries and gets 8-query packets, which exist for the per-lane lists and
    k <= 20 only: k_knn_cov<20, REG, 2, true> whatever k <= 20 is (KMAX 20 with sentinel slots), every packet behind a borrowed window of >= 32 points.  With
    the gather forced to 0 or 1, or k > 20, the engine falls back to 32-query packets: the same launch as under "32".

tests/test_knn_trim_gpu.py runs the checks on the MI355X,
tests/test_knn_trim_simt_host.py on the host emulation of the same kernels.  `make_engine(params)` builds a RegistrationHIP on the library under test.
Inputs are seeded, computed once and read-only."""
from __future__ import annotations

import contextlib
import functools
import os

import numpy as np

import oracle as O
import parity_checks as PC
import prefilter_checks as PFC
from hdl_graph_slam_amd import synth

PACKET_RULES = {"32": "knn_qpw_tiny=0", "tiered": "knn_qpw_tiny=-1"}
# Under "32" (32-query packets, window = the packet): 1 .. 21 are one packet and the whole cloud — no walk, windows of 1, 7, 9, 19 (odd: tail iteration),
# 20 (even) and 21 points, fewer points than k = 20 (lists never fill, found < k), exactly k, k + 1, the one-leaf (1, 7) and two-leaf (9) trees; 63 is a full
# packet and one of 31 (an odd window of more than one point in front of a walk), 64 two full packets, 65 / 129 / 2049 end in a packet of one point (63 idle
# lanes); 75 ends in one of 11.  Under "tiered" (8-query packets, borrowed window): n <= 32 is a window that is the whole cloud (no walk, odd and even counts),
# 63 / 65 / 75 / 129 end in packets of 7 / 1 / 3 / 1 points behind windows of 32 .. 39 points.
CLOUD_SIZES = (1, 7, 9, 19, 20, 21, 63, 64, 65, 75, 129, 2049)
# Under "32": every KMAX instantiation at its bound (8, 16, 20, 32, 64) and lists whose low slots hold the -1 sentinel (1 and 5 in KMAX 8, 17 in 20).  Under
# "tiered": k <= 20 all run KMAX 20 with 19 .. 0 sentinel slots in the short-packet kernel; 32 and 64 are the "32" launches again.
K_VALUES = (1, 5, 8, 16, 17, 20, 32, 64)
K_CLOUDS = (129, 2049)
GATHER_MODES = ("0", "1", "2")


def _frozen(cloud: np.ndarray) -> np.ndarray:
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def random_cloud(n: int) -> np.ndarray:
    rng = np.random.default_rng(3000 + n)
    return _frozen(synth.to_xyzi(rng.uniform(-3, 3, (n, 3)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def duplicated_cloud() -> np.ndarray:
    """150 random points, each one twice (shuffled): every query has a neighbour at distance 0 besides itself, every k-th distance is shared by two points."""
    rng = np.random.default_rng(41)
    xyz = rng.uniform(-2, 2, (150, 3)).astype(np.float32)
    return _frozen(synth.to_xyzi(np.concatenate([xyz, xyz])[rng.permutation(300)]))


@functools.lru_cache(maxsize=None)
def tie_heavy() -> np.ndarray:
    return _frozen(PC.tie_heavy_cloud())


@functools.lru_cache(maxsize=None)
def nonfinite_cloud() -> np.ndarray:
    """301 random points of which every fourth is non-finite (NaN in x, +inf in y, -inf in z in turn): they are dropped, the 225 that remain end in a
    leaf with pad points, whose +inf distances reach the chain."""
    cloud = random_cloud(301).copy()
    cloud["x"][0::12] = np.nan
    cloud["y"][4::12] = np.inf
    cloud["z"][8::12] = -np.inf
    return _frozen(cloud)


@functools.lru_cache(maxsize=None)
def huge_coordinate_cloud() -> np.ndarray:
    """300 ordinary points around the origin, 30 points around (1e18, -1e18, 1e18), and 30 each around x = +1.2e19 and x = -1.2e19.  Squared distances from
    the origin to the first cluster are ~3e36 (finite); between the two outer clusters they are (2.4e19)^2 = 5.8e38 > FLT_MAX: +inf in float.  Inside a
    cluster the points are a few thousand float steps apart (one step is 6.9e10 at 1e18, 1.1e12 at 1.2e19), so every cluster member has its 20 nearest in
    its own cluster at finite distances and a finite covariance (~1e28)."""
    rng = np.random.default_rng(43)
    near = rng.uniform(-3, 3, (300, 3)).astype(np.float32)

    def cluster(centre, step):
        return (np.asarray(centre, np.float64) + step * rng.integers(-4000, 4000, (30, 3))).astype(np.float32)

    pts = np.concatenate([near, cluster([1e18, -1e18, 1e18], 6.9e10), cluster([1.2e19, 0.0, 0.0], 1.1e12), cluster([-1.2e19, 0.0, 0.0], 1.1e12)])
    return _frozen(synth.to_xyzi(pts[rng.permutation(len(pts))]))


@contextlib.contextmanager
def engine_options(options: str):
    """HGS_ENGINE_OPTIONS for the engines created inside (the harness applies it when an engine is created)."""
    old = os.environ.get("HGS_ENGINE_OPTIONS")
    os.environ["HGS_ENGINE_OPTIONS"] = options
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("HGS_ENGINE_OPTIONS", None)
        else:
            os.environ["HGS_ENGINE_OPTIONS"] = old


def covariances_match(make_engine, cloud, k=20, method=O.HGS_REG_FROBENIUS):
    """The engine's covariances of `cloud` as a target against the oracle's (PC.check_covariances); none may be NaN or infinite.  Returns them."""
    p = O.default_params(O.HGS_FAST_GICP)
    p.correspondence_randomness = k
    p.regularization_method = method
    e = make_engine(p)
    try:
        e.setInputTarget(cloud)
        PC.check_covariances(e, cloud, k, method)
        got = e.target_covariances(len(cloud)).copy()
    finally:
        e.close()
    assert np.isfinite(got).all(), "non-finite covariance"
    return got


def check_cloud_size(make_engine, n: int, rule: str):
    """One cloud size under the engine's own gather (the per-lane lists) and, under "32" where there is a walk to gather from, the two others (under "tiered" a
    forced gather 0 / 1 is the "32" launch)."""
    cloud = random_cloud(n)
    with engine_options(PACKET_RULES[rule]):
        got = covariances_match(make_engine, cloud)
    assert got.any(axis=1).all()                              # every point got a covariance
    if rule == "32" and n > 32:
        for mode in ("0", "1"):
            with engine_options(PACKET_RULES[rule] + ",knn_replay=" + mode):
                covariances_match(make_engine, cloud)


def check_k(make_engine, n: int, k: int, rule: str):
    with engine_options(PACKET_RULES[rule]):
        covariances_match(make_engine, random_cloud(n), k)


def check_regularization(make_engine, method_name: str, split: int, gather_mode: str, rule: str):
    """FROBENIUS (REG 0) and PLANE with the eigen-decomposition inline (cov_split=0: REG 1) or staged (cov_split=1: REG 2 + k_cov_regularize), under each gather
    mode, on 2049 points: k_knn_cov<20, REG, GATHER, false> under "32"; under "tiered" gather 2 is k_knn_cov<20, REG, 2, true> (0 and 1 repeat "32")."""
    method = {"FROBENIUS": O.HGS_REG_FROBENIUS, "PLANE": O.HGS_REG_PLANE}[method_name]
    with engine_options(f"{PACKET_RULES[rule]},cov_split={split},knn_replay={gather_mode}"):
        covariances_match(make_engine, random_cloud(2049), 20, method)


def check_ties(make_engine, which: str, gather_mode: str, rule: str):
    """Several points at exactly the k-th distance: candidates whose distance EQUALS the lane's worst must not move its list (they are the gather
    pass's to choose from by original index), and lanes that need several of them run the TIES = 4 walk."""
    cloud = {"duplicated": duplicated_cloud, "tie_heavy": tie_heavy}[which]()
    with engine_options(PACKET_RULES[rule] + ",knn_replay=" + gather_mode):
        covariances_match(make_engine, cloud)
        if which == "duplicated":
            covariances_match(make_engine, cloud, 5)          # sentinel slots next to exact duplicates (KMAX 8 under "32")
            covariances_match(make_engine, cloud, 16)         # a full KMAX 16 list under "32"


def check_nonfinite_input(make_engine, rule: str):
    cloud = nonfinite_cloud()
    with engine_options(PACKET_RULES[rule]):
        got = covariances_match(make_engine, cloud)
    finite = np.isfinite(cloud["x"]) & np.isfinite(cloud["y"]) & np.isfinite(cloud["z"])
    assert 0 < finite.sum() < len(cloud) and (finite.sum() % 8) != 0            # points are dropped and the last leaf has pad points
    assert got[finite].any(axis=1).all() and not got[~finite].any()


def check_huge_coordinates(make_engine, rule: str):
    cloud = huge_coordinate_cloud()
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
    with np.errstate(over="ignore"):
        d2 = ((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1, dtype=np.float32)
    assert np.isinf(d2).any() and not np.isnan(d2).any()                          # what the case is built for: +inf distances, no NaN
    for mode in GATHER_MODES:
        with engine_options(PACKET_RULES[rule] + ",knn_replay=" + mode):
            covariances_match(make_engine, cloud)


def check_far_outliers(make_engine, rule: str):
    """PC.outlier_cloud at k = 20 and 48: packets over sparse far returns, walks of hundreds of leaves, leaf lists and logs that overflow (the gather
    then walks the tree).  "32": k_knn_cov<20, 0, 2, false> and <64, 0, 2, false>; "tiered": <20, 0, 2, true> at k = 20 (k = 48 repeats "32")."""
    with engine_options(PACKET_RULES[rule]):
        PC.check_covariances_with_outliers(make_engine)


def check_short_packets(make_engine, qpw: int):
    """8- / 16-query packets (k_knn_cov<20, REG, 2, true>: every packet borrows a pre-fill window of >= 32 points) on 300 points; 297: a last packet of one
    point behind an odd window."""
    with engine_options(f"knn_qpw_tiny={qpw},knn_replay=2"):
        for n in (300, 297):
            covariances_match(make_engine, random_cloud(n))
            covariances_match(make_engine, random_cloud(n), 17)


def check_statistical_outlier_removal(make_engine):
    """hgs_prefilter's statistical outlier removal on 4097 points (k_pf_mean_knn_dist: KnnRadiusLane under the generic packet walk, idle lanes parked at
    FLT_MAX), point for point against the oracle."""
    cloud = PFC.mixture(4097, 3)
    reg = make_engine(O.default_params(O.HGS_FAST_GICP))
    try:
        for mean_k in (20, 15):                               # KMAX 32 with sentinel slots, KMAX 16 full
            got = PFC.expect_oracle(reg, cloud, PFC._stat(mean_k=mean_k), f"statistical mean_k={mean_k}")
            assert 0 < len(got) < len(cloud)
    finally:
        reg.close()
