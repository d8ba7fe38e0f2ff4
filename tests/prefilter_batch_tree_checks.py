"""Shared checks of hgs_prefilter_batch under the parameter sets whose outlier removal needs a search tree per sweep (STATISTICAL; RADIUS without a voxel
grid, with radius / leaf > 4 or with prefilter_fast = 0): the batched tail of prefilter_batch_impl (hgs_engine.hip) and the k_pfb_radius_flags /
k_pfb_mean_knn_dist / k_pfb_dist_stats / k_pfb_statistical_flags kernels (hgs_kernels.hip).  tests/test_prefilter_batch_tree_gpu.py runs them on the MI355X,
tests/test_prefilter_batch_tree_simt_host.py on the host emulation of the same kernels.  `make_engine()` builds a RegistrationHIP (FAST_GICP) on the library
under test.

The yardstick is the single call, as in tests/prefilter_batch_checks.py, whose sweep set, plumbing and references these checks share: out[i] of the batch
against hgs_prefilter_framed(sweep i) on a FRESH engine.  Every comparison is of BITS: there is no tolerance anywhere in this file.

The sweeps: the seven of prefilter_batch_checks.sweeps() and an eighth, sweep_a()[300:310] — ten neighbouring returns, a cloud that reaches the tree stage
with between 2 and mean_k points (every k-nearest search finds fewer than mean_k + 1, the sums are still divided by mean_k).  On the CPU oracle
(check_counts_against_the_oracle) the eighth sweep gives 3 points under `statistical` (4 voxels at leaf 0.25 reach the tree stage, one lies beyond the
threshold), 10 under `radius_no_grid`, 8 under `vg010_radius`; without a voxel grid or distance filter (`stat_raw`) all 10 reach the tree stage and 9 stay.

statistical_mean_k = 63 is refused by hgs_prefilter_params' check (1 .. 62: tests/prefilter_checks.py::check_arguments pins it), by the single call and by
the batch alike, so the largest instantiation k_pfb_mean_knn_dist<64> runs at 62 here; for 63 the checks ask that the batch refuses what the single call
refuses and reproduce the oracle's counts on the CPU only."""
from __future__ import annotations

import functools

import numpy as np

import oracle as O
import prefilter_batch_checks as BC
import prefilter_checks as PFC
from prefilter_batch_checks import NONE, RADIUS, STATISTICAL, Sweep, same_bits, downloaded, single_cloud, batch_clouds

_STAT = dict(downsample_resolution=0.25, outlier_removal_method=STATISTICAL)
# name -> (hgs_prefilter_params fields over the nodelet's defaults, the engine's prefilter_fast option); the first four are prefilter_batch_checks'
CONFIGS = {k: BC.CONFIGS[k] for k in ("statistical", "radius_no_grid", "vg010_radius", "slow_vg025_radius")}
CONFIGS.update({
    "stat_k5": (dict(_STAT, statistical_mean_k=5, statistical_stddev=0.5), 1),         # k_pfb_mean_knn_dist<16>
    "stat_k40": (dict(_STAT, statistical_mean_k=40, statistical_stddev=1.0), 1),       # <64>
    "stat_k62": (dict(_STAT, statistical_mean_k=62, statistical_stddev=2.0), 1),       # <64>, the largest mean_k the interface takes
    "stat_raw": (dict(use_distance_filter=0, downsample_method=NONE, outlier_removal_method=STATISTICAL, statistical_mean_k=20), 1),
    "radius_raw": (dict(use_distance_filter=0, downsample_method=NONE, outlier_removal_method=RADIUS, radius_radius=0.8, radius_min_neighbors=1), 1),
})
TREE = ("statistical", "radius_no_grid", "vg010_radius", "slow_vg025_radius")
STAT_K63 = dict(_STAT, statistical_mean_k=63, statistical_stddev=2.0)

# the CPU oracle's output counts, sweeps 1-7 of prefilter_batch_checks.sweeps() (oracle.prefilter; reproduced by check_counts_against_the_oracle)
ORACLE_COUNTS = {
    "statistical": (1559, 0, 1554, 0, 1, 1210, 54),
    "radius_no_grid": (2826, 0, 2826, 0, 0, 1439, 255),
    "vg010_radius": (2272, 0, 2272, 0, 0, 1433, 150),
    "stat_k5": (1546, 0, 1540, 0, 1, 1147, 48),
    "stat_k40": (1539, 0, 1535, 0, 1, 1217, 53),
}
ORACLE_COUNTS_K63 = (1558, 0, 1553, 0, 1, 1242, 62)
ORACLE_COUNTS_SWEEP8 = {"statistical": 3, "radius_no_grid": 10, "vg010_radius": 8, "stat_raw": 9}
# sweep A and A + 0.3 m as ONE cloud against the sum of the two alone
ORACLE_ONE_CLOUD = {"statistical": (2667, 1559 + 1554), "radius_no_grid": (5988, 5652), "vg010_radius": (4388, 4544)}


@functools.lru_cache(maxsize=None)
def sweeps() -> tuple:
    return BC.sweeps() + (Sweep(BC.sweep_a()[300:310].copy()),)                        # 8 fewer points than mean_k at the tree stage


ALL = tuple(range(8))


def params_of(config):
    return PFC.device_params(**CONFIGS[config][0])


def engine_for(make_engine, config, tree=1):
    reg = make_engine()
    reg.set_option("prefilter_fast", CONFIGS[config][1])
    reg.set_option("prefilter_batch_tree", tree)
    return reg


_REFERENCE = {}


def reference(make_engine, config, i) -> np.ndarray:
    """The single call for sweep i on a fresh engine (computed once per library under test, read-only; shared with prefilter_batch_checks where it has it)."""
    if config in BC.CONFIGS and i < len(BC.sweeps()):
        return BC.reference(make_engine, config, i)
    key = (make_engine.__module__, config, i)
    if key not in _REFERENCE:
        reg = make_engine()
        reg.set_option("prefilter_fast", CONFIGS[config][1])
        out = downloaded([single_cloud(reg, sweeps()[i], params_of(config))])[0]
        reg.close()
        out.setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]


def assert_batch_equals_reference(make_engine, reg, config, idx, label=""):
    got = downloaded(batch_clouds(reg, [sweeps()[i] for i in idx], params_of(config)))
    assert len(got) == len(idx)
    for k, i in enumerate(idx):
        same_bits(got[k], reference(make_engine, config, i), (config, label, "sweep", i + 1))
    return got


def stats_after_batch(reg, config, idx) -> dict:
    for c in batch_clouds(reg, [sweeps()[i] for i in idx], params_of(config)):
        c.close()
    return reg.prefilter_batch_stats()


# ---- 1. the path is taken
def check_path_is_taken(make_engine):
    """The batch sequence runs the tree-based parameter sets: two read-backs, one index build and one tree-walk launch whatever S is."""
    for config in TREE:
        reg = engine_for(make_engine, config)
        for idx in (ALL, (0, 5, 6)):
            st = stats_after_batch(reg, config, idx)
            assert st == dict(sweeps=len(idx), batched=1, readbacks=2, index_builds=1, tree_launches=1), (config, idx, st)
        reg.set_option("prefilter_batch_tree", 0)
        st = stats_after_batch(reg, config, ALL)
        # sweep after sweep: a read-back per sweep, and an index build + a second read-back per sweep that reaches the tree stage with points
        assert st["batched"] == 0 and st["tree_launches"] == 0 and st["index_builds"] > 1 and st["readbacks"] == 8 + st["index_builds"], (config, st)
        reg.close()
    reg = make_engine()
    assert reg.prefilter_batch_stats() == dict(sweeps=0, batched=0, readbacks=0, index_builds=0, tree_launches=0)
    for c in batch_clouds(reg, sweeps(), BC.params_of("vg025_radius")):
        c.close()
    st = reg.prefilter_batch_stats()
    assert (st["batched"], st["index_builds"], st["readbacks"], st["tree_launches"]) == (1, 0, 1, 0), st            # the grid path is untouched
    for c in batch_clouds(reg, sweeps(), BC.params_of("approx")):
        c.close()
    assert reg.prefilter_batch_stats()["batched"] == 0
    st = stats_after_batch(reg, "statistical", (1, 3))                      # every sweep empty behind the front: the tail is skipped
    assert (st["batched"], st["index_builds"], st["readbacks"], st["tree_launches"]) == (1, 0, 1, 0), st
    st = stats_after_batch(reg, "statistical", (0,))                        # S = 1: the single sequence
    assert (st["sweeps"], st["batched"], st["index_builds"], st["readbacks"]) == (1, 0, 1, 2), st
    reg.close()


# ---- 2. bit equality with the single call on a fresh engine, and of both values of prefilter_batch_tree
def check_batch_equals_single_calls(make_engine, config):
    reg = engine_for(make_engine, config)
    got = assert_batch_equals_reference(make_engine, reg, config, ALL)
    assert reg.prefilter_batch_stats()["batched"] == 1
    assert len(got[1]) == 0 and len(got[0]) > 1000
    reg.set_option("prefilter_batch_tree", 0)
    each = downloaded(batch_clouds(reg, sweeps(), params_of(config)))
    assert reg.prefilter_batch_stats()["batched"] == 0
    for i in ALL:
        same_bits(got[i], each[i], (config, "prefilter_batch_tree 1 against 0", "sweep", i + 1))
    if config in ("stat_raw", "radius_raw"):                                # sweep A's two non-finite records reached the tree stage and are gone
        a = BC.sweep_a()
        assert np.isfinite(a["y"]).sum() == len(a) - 1 and np.isfinite(a["x"]).sum() == len(a) - 1
        for f in ("x", "y", "z"):
            assert np.isfinite(got[0][f]).all() and np.isfinite(got[2][f]).all()
    reg.close()


def check_mean_k_63_is_refused_alike(make_engine):
    """statistical_mean_k = 63 lies outside the interface's 1 .. 62: the batch refuses it as the single call does, and writes nothing."""
    from hdl_graph_slam_amd import _lib as L
    reg = make_engine()
    assert PFC.prefilter_status(reg, BC.sweep_a(), STAT_K63) == L.HGS_ERR_INVALID_ARGUMENT
    entries = [BC.entry(s) for s in sweeps()]
    rc, out = BC.raw_batch(reg, [e[0] for e in entries], PFC.device_params(**STAT_K63))
    assert rc == L.HGS_ERR_INVALID_ARGUMENT and all(v == 0xdead for v in out), (rc, out)
    reg.close()


# ---- 3. a sweep sees its own points only, and the inputs can show it
@functools.lru_cache(maxsize=None)
def oracle_counts(config) -> tuple:
    fields = STAT_K63 if config == "stat_k63" else CONFIGS[config][0]
    return tuple(len(O.prefilter(s.cloud, PFC.oracle_params(**fields))) for s in sweeps())


def check_counts_against_the_oracle(make_engine):
    """The figures of the CPU oracle, reproduced here first; then the batch's counts are those figures.  The oracle knows no mount matrix: both sides take
    the sweeps' points without their gyro samples and mounts."""
    for config, want in ORACLE_COUNTS.items():
        assert oracle_counts(config)[:7] == want, (config, oracle_counts(config))
    assert oracle_counts("stat_k63")[:7] == ORACLE_COUNTS_K63, oracle_counts("stat_k63")
    for config, want in ORACLE_COUNTS_SWEEP8.items():
        assert oracle_counts(config)[7] == want, (config, oracle_counts(config))
    a, b = BC.sweep_a(), BC.shifted(BC.sweep_a(), 0.3)
    for config, (one, alone) in ORACLE_ONE_CLOUD.items():
        p = PFC.oracle_params(**CONFIGS[config][0])
        assert (len(O.prefilter(np.concatenate([a, b]), p)), len(O.prefilter(a, p)) + len(O.prefilter(b, p))) == (one, alone), config
        assert one != alone           # statistics or neighbour counts that reached into the neighbouring slice could not give the single calls' clouds
    for config in list(ORACLE_COUNTS) + ["stat_k62", "stat_raw"]:
        reg = engine_for(make_engine, config)
        got = batch_clouds(reg, [Sweep(s.cloud) for s in sweeps()], params_of(config))
        assert tuple(c.size for c in got) == oracle_counts(config), (config, [c.size for c in got])
        for c in got:
            c.close()
        reg.close()


# ---- 4. calls back to back on one engine; the handle's target and source
def check_back_to_back(make_engine):
    reg = engine_for(make_engine, "statistical")
    assert_batch_equals_reference(make_engine, reg, "statistical", ALL, "first call: a tree batch")
    BC.assert_batch_equals_reference(make_engine, reg, "vg025_radius", BC.ALL, "second call: a grid batch")
    same_bits(downloaded([single_cloud(reg, sweeps()[5], params_of("statistical"))])[0], reference(make_engine, "statistical", 5), "the single call between them")
    assert_batch_equals_reference(make_engine, reg, "vg010_radius", (6, 2, 7, 2, 4), "fourth call: fewer sweeps, another order, one sweep twice")
    assert reg.prefilter_batch_stats() == dict(sweeps=5, batched=1, readbacks=2, index_builds=1, tree_launches=1)
    assert_batch_equals_reference(make_engine, reg, "statistical", (7, 0), "fifth call")
    reg.close()


def check_handle_state(make_engine):
    reg = engine_for(make_engine, "statistical")
    p = BC.params_of("vg025_none")
    tgt, src = single_cloud(reg, sweeps()[0], p), single_cloud(reg, sweeps()[2], p)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    before = reg.align(np.eye(4, dtype=np.float32))
    assert_batch_equals_reference(make_engine, reg, "statistical", ALL)
    assert_batch_equals_reference(make_engine, reg, "radius_no_grid", ALL)
    after = reg.align(np.eye(4, dtype=np.float32))
    assert bytes(before) == bytes(after) and before.iterations > 0
    reg.close()


# ---- 5. failure leaves nothing behind
def check_overflow_leaves_nothing(make_engine):
    """One point 3e8 m away at leaf 0.1 in the third sweep of a STATISTICAL batch: the call fails at read-back 1, names the sweep, every out[i] is NULL,
    and the caller's clouds cost what they cost before."""
    from hdl_graph_slam_amd import _lib as L
    fields = dict(CONFIGS["statistical"][0], use_distance_filter=0, downsample_resolution=0.1)
    reg = engine_for(make_engine, "statistical")
    held = batch_clouds(reg, sweeps(), params_of("statistical"))
    before = [c.device_bytes for c in held]
    s = sweeps()
    entries = [BC.entry(s[0]), BC.entry(s[7]), BC.entry(Sweep(BC.overflowing_sweep().copy())), BC.entry(s[5])]
    rc, out = BC.raw_batch(reg, [e[0] for e in entries], PFC.device_params(**fields))
    assert rc == L.HGS_ERR_INVALID_ARGUMENT, rc
    msg = L.lib().hgs_last_error(reg._h).decode()
    assert "too fine" in msg and "sweep 2" in msg, msg
    assert out == [0, 0, 0, 0], out
    assert reg.prefilter_batch_stats() == dict(sweeps=4, batched=1, readbacks=1, index_builds=0, tree_launches=0)
    assert [c.device_bytes for c in held] == before and sum(before) > 0
    for k, c in enumerate(downloaded(held)):
        same_bits(c, reference(make_engine, "statistical", k), ("held across the failed call", k + 1))
    assert_batch_equals_reference(make_engine, reg, "statistical", ALL, "after the failed call")
    reg.close()


# ---- 6. downstream
def check_downstream_use(make_engine):
    reg = engine_for(make_engine, "statistical")
    p = params_of("statistical")
    idx = (0, 2, 5)
    singles = [single_cloud(reg, sweeps()[i], p) for i in idx]
    every = batch_clouds(reg, sweeps(), p)
    assert reg.prefilter_batch_stats()["batched"] == 1
    batch = [every[i] for i in idx]
    guesses = [np.eye(4, dtype=np.float32)] * 3
    order = (1, 0, 2)
    want = reg.align_pairs([singles[t] for t in order], singles, guesses, max_range=2.0)
    got_sources = reg.align_pairs([singles[t] for t in order], batch, guesses, max_range=2.0)
    got_both = reg.align_pairs([batch[t] for t in order], batch, guesses, max_range=2.0)
    assert want["iterations"][0] > 0 and want["num_inliers"].min() > 100
    assert want.tobytes() == got_sources.tobytes() == got_both.tobytes()
    reg.setInputTarget(batch[0])
    reg.setInputSource(batch[1])
    got = reg.align(np.eye(4, dtype=np.float32))
    reg.setInputTarget(singles[0])
    reg.setInputSource(singles[1])
    assert bytes(got) == bytes(reg.align(np.eye(4, dtype=np.float32))) and got.iterations > 0
    for c in singles + every:
        c.close()
    reg.close()


def check_lockstep_odometry(make_engine):
    """Two streams of raw sweeps (every 8th ray of a VLP-16), three sweep times, STATISTICAL behind a 1 m voxel grid: LockstepOdometry's poses are bytewise
    those of two ScanMatchingOdometry fed by single prefilter calls, and every step's prefilter ran as one batch."""
    from hdl_graph_slam_amd import synth
    from hdl_graph_slam_amd.odometry import LockstepOdometry, ScanMatchingOdometry
    p = PFC.device_params(downsample_resolution=1.0, outlier_removal_method=STATISTICAL, statistical_mean_k=20, statistical_stddev=1.0)
    mounts = [BC.T_LIFT, None]
    kw = dict(keyframe_delta_trans=0.5, keyframe_delta_angle=10.0, keyframe_delta_time=100.0)
    raw = [[synth.scan(synth.make_scene(21 + s), "VLP-16", synth.pose_matrix([v * k, 0.02 * k, 0.0], [0.0, 0.0, 0.004 * k * (s + 1)]), 300 + 10 * s + k)[::8].copy()
            for k in range(3)] for s, v in enumerate((0.12, 0.3))]
    single = []
    for s in range(2):
        e = make_engine()
        od = ScanMatchingOdometry(e, downsample=lambda c, e=e, s=s: e.prefilter(c, p, base_link_transform=mounts[s]), **kw)
        single.append([od.matching(0.1 * k, raw[s][k]).tobytes() for k in range(3)])
        e.close()
    assert len({x for poses in single for x in poses}) > 3                  # the streams move
    e = make_engine()
    lock = LockstepOdometry(e, 2, prefilter_params=p, base_link_transforms=mounts, **kw)
    for k in range(3):
        odoms = lock.matching(0.1 * k, [raw[s][k] for s in range(2)])
        st = e.prefilter_batch_stats()
        assert (st["sweeps"], st["batched"], st["readbacks"], st["index_builds"]) == (2, 1, 2, 1), (k, st)
        for s in range(2):
            assert odoms[s].tobytes() == single[s][k], (s, k)
    e.close()
