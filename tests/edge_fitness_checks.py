"""Shared checks of hgs_calc_fitness_score_batch — the fitness scores of all edges of one graph update in one device batch
(flush_keyframe_queue and the loop step, apps/hdl_graph_slam_nodelet.cpp:235,569) — run on an MI355X (tests/test_edge_fitness_gpu.py) and on the
same kernels emulated on the host (tests/test_edge_fitness_simt_host.py).  The yardstick is exact: a pair's score depends on its own two clouds
and its pose only, so every score of the batch equals, bit for bit, what hgs_calc_fitness_score returns for that pair on a FRESH engine; the
seed grids of the batched build are read back (hgs_debug_cloud_seed_grid) and compared word for word with the single-cloud build's, because a
wrong seed table never changes a score."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import sys

import numpy as np

from hdl_graph_slam_amd import _lib as L, synth
from hdl_graph_slam_amd.information_matrix import InformationMatrixCalculator
from hdl_graph_slam_amd.registration import RegistrationHIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "golden")) if p not in sys.path]

DBL_MAX = L.DBL_MAX
FIT_RTOL = 2e-6      # tests/test_reference_code_pins.py: measured, oracle 1.2e-7 (the two PCL orders differ from each other by 2.8e-7)
METHODS = {"FAST_GICP": L.HGS_FAST_GICP, "NDT_OMP": L.HGS_NDT_OMP}
RANGES = (DBL_MAX, 1.0, 1e-9)
GOLDEN = os.path.join(ROOT, "tests", "golden", "refpin_v1.npz")


def make_engine(method="FAST_GICP", seed_grid=1):
    e = RegistrationHIP(L.default_params(METHODS[method]))
    e.set_option("seed_grid", seed_grid)
    return e


class Scene:
    """Five keyframes along a corridor (VLP-16 scans voxel-downsampled at 1.0: several hundred points each), one scan of several thousand points,
    and hand-made tiny clouds.  The pair list — (tree, query, pose) — of ONE call:
      0      the large scan against keyframe 0
      1..4   the chain: keyframe i is the tree of pair i and the query of pair i + 1
      5      pair 2 again
      6      pair 2 with the roles swapped
      7      keyframe 3 against itself at the identity: score 0.0, every point an inlier
      8..11  queries of 1, 63, 256 and 257 points (k_fitness: tiles of 256 points, packets of 64) — next to the large one, their blocks beyond their tiles return
      12,13  trees of 1 point and of 9 points (leaves hold 8)
      14     a query with non-finite records"""

    def __init__(self):
        sc = synth.make_scene(5)
        rng = np.random.default_rng(23)
        self.clouds, self.poses = {}, {}

        def frame(name, x, seed, leaf):
            pose = synth.pose_matrix([x, 0.1 * np.sin(x), 0.0], [0.0, 0.0, 0.03 * x])
            self.clouds[name] = synth.voxel_downsample(synth.scan(sc, "VLP-16", pose, seed), leaf)
            self.poses[name] = pose @ synth.pose_matrix(rng.normal(0, 0.05, 3) * [1, 1, 0], [0.0, 0.0, rng.normal(0, 0.005)])   # odometry: a little drift

        for i in range(5):
            frame(f"k{i}", -2.0 + i, 300 + i, 1.0)
        frame("big", -2.4, 310, 0.3)
        k1, k2 = self.clouds["k1"], self.clouds["k2"]
        for n in (1, 63, 256, 257):
            self.clouds[f"q{n}"] = np.ascontiguousarray(k1[3::2][:n])
            self.poses[f"q{n}"] = self.poses["k1"]
        for n in (1, 9):
            self.clouds[f"t{n}"] = np.ascontiguousarray(k2[11::7][:n])
            self.poses[f"t{n}"] = self.poses["k2"]
        bad = k1.copy()
        bad["x"][[5, 100, len(bad) - 1]] = np.nan
        bad["y"][[7, 64]] = np.inf
        bad["z"][200] = -np.inf
        self.clouds["nan"], self.poses["nan"] = bad, self.poses["k1"]
        self.n_nonfinite = 6
        names = [("k0", "big")] + [(f"k{i}", f"k{i - 1}") for i in range(1, 5)] + [("k2", "k1"), ("k1", "k2"), ("k3", "k3")]
        names += [("k0", f"q{n}") for n in (1, 63, 256, 257)] + [("t1", "k1"), ("t9", "k1"), ("k2", "nan")]
        self.pairs = names
        # the pose of an edge: cloud2 in cloud1's frame (information_matrix_calculator.cpp:63 moves cloud2 by relpose)
        self.relposes = [np.eye(4, dtype=np.float32) if a == b else (np.linalg.inv(self.poses[a]) @ self.poses[b]).astype(np.float32) for a, b in names]
        sizes = {k: len(v) for k, v in self.clouds.items()}
        assert sizes["big"] >= 3000 and all(300 <= sizes[f"k{i}"] <= 3000 for i in range(5)), sizes
        assert [sizes[f"q{n}"] for n in (1, 63, 256, 257)] == [1, 63, 256, 257] and sizes["t1"] == 1 and sizes["t9"] == 9, sizes


@functools.lru_cache(maxsize=None)
def scene() -> Scene:
    return Scene()


_reference = {}


def reference(method, seed_grid, max_range):
    """[(score, inliers) per pair of the scene]: hgs_calc_fitness_score on a FRESH engine per pair; the inlier count of the single path read through
    setInputTarget / setInputSource / getFitnessScore -> last_num_inliers behind it.  Computed once per setting and library."""
    key = (L.LIB_PATH, method, seed_grid, max_range)
    if key not in _reference:
        s = scene()
        out = []
        for (a, b), T in zip(s.pairs, s.relposes):
            e = make_engine(method, seed_grid)
            da = e.upload(s.clouds[a])
            db = da if a == b else e.upload(s.clouds[b])
            score = e.calc_fitness_score(da, db, T, max_range)
            e.setInputTarget(da)
            e.setInputSource(db)
            assert e.getFitnessScore(max_range, T=T) == score, (a, b)
            out.append((score, e.last_num_inliers))
            da.close(), db.close()
            e.close()
        _reference[key] = out
    return _reference[key]


class Case:
    """One engine with the scene's clouds resident."""

    def __init__(self, method="FAST_GICP", seed_grid=1):
        self.method, self.seed_grid = method, seed_grid
        self.e = make_engine(method, seed_grid)
        self.dev = {k: self.e.upload(v) for k, v in scene().clouds.items()}

    def pairs(self, which=None):
        s = scene()
        idx = range(len(s.pairs)) if which is None else which
        return [(self.dev[s.pairs[i][0]], self.dev[s.pairs[i][1]], s.relposes[i]) for i in idx]

    def close(self):
        for c in self.dev.values():
            c.close()
        self.e.close()


def bits(a):
    return np.asarray(a, np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ 1: bit equality with the single call
def check_scores_equal_single_calls(method, seed_grid):
    s = scene()
    for max_range in RANGES:
        case = Case(method, seed_grid)          # a fresh batch engine per range: every call builds its own indices and seed grids
        scores, inliers = case.e.calc_fitness_scores(case.pairs(), max_range, return_inliers=True)
        ref = reference(method, seed_grid, max_range)
        for i, ((a, b), (rs, rn)) in enumerate(zip(s.pairs, ref)):
            assert bits(scores[i]) == bits(rs) and int(inliers[i]) == rn, (method, seed_grid, max_range, i, a, b, float(scores[i]).hex(), float(rs).hex(), inliers[i], rn)
        if max_range == 1e-9:
            # (pair 7, a cloud against itself, has d2 = 0 <= 1e-9 for every point: the one exception the range leaves)
            keep = [i for i in range(len(s.pairs)) if i != 7]
            assert (scores[keep] == DBL_MAX).all() and (inliers[keep] == 0).all(), (scores, inliers)
        elif max_range == DBL_MAX:
            assert (scores < DBL_MAX).all() and (inliers > 0).all(), (scores, inliers)
        else:                                   # 1 m2: a range that divides the points of most pairs
            part = [i for i in range(len(s.pairs)) if 0 < inliers[i] < len(s.clouds[s.pairs[i][1]])]
            assert len(part) >= 8, (inliers, part)
        assert scores[7] == 0.0 and inliers[7] == len(s.clouds["k3"])
        if max_range == DBL_MAX:
            assert inliers[14] == len(s.clouds["nan"]) - s.n_nonfinite and inliers[0] == len(s.clouds["big"]), inliers
            assert bits(scores[5]) == bits(scores[2]) and bits(scores[6]) != bits(scores[2])
        # a second call on the same engine (everything cached now) returns the same bits
        again, again_n = case.e.calc_fitness_scores(case.pairs(), max_range, return_inliers=True)
        assert bits(again) == bits(scores) and (again_n == inliers).all()
        case.close()


# ------------------------------------------------------------------------------------------------ 2: the reference's own numbers
def check_against_reference_vectors(method):
    import make_refpin_golden as MG
    gold = np.load(GOLDEN)
    clouds = MG.small_clouds()[0]
    e = make_engine(method)
    dev = {k: e.upload(c) for k, c in clouds.items() if len(c)}
    records = [i for i in range(len(gold["fit_score"])) if str(gold["fit_cloud2"][i]) != "empty"]
    assert len(records) == len(gold["fit_score"]) - 1 >= 20
    run, worst = 0, 0.0
    for r in sorted(set(float(v) for v in gold["fit_max_range"])):
        group = [i for i in records if float(gold["fit_max_range"][i]) == r]
        scores = e.calc_fitness_scores([(dev[str(gold["fit_cloud1"][i])], dev[str(gold["fit_cloud2"][i])], gold["fit_pose"][i]) for i in group], r)
        for i, s in zip(group, scores):
            ref = float(gold["fit_score"][i])
            run += 1
            if ref == DBL_MAX:
                assert s == DBL_MAX, i
            else:
                dev_i = abs(float(s) / ref - 1)
                worst = max(worst, dev_i)
                assert dev_i < FIT_RTOL, (i, float(s), ref, dev_i)
    assert run == len(records)
    print(f"{method}: {run} records, worst relative deviation {worst:.3g}")
    for c in dev.values():
        c.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 3: seed tables
SEED_CLOUDS = ("big", "k0", "k1", "k2", "k3", "q63")      # several thousand ... several hundred points, one below 64


def _single_build_table(name):
    """The seed grid of one cloud on a fresh engine that built it through one hgs_calc_fitness_score."""
    s = scene()
    e = make_engine()
    c, q = e.upload(s.clouds[name]), e.upload(s.clouds["q1"])
    e.calc_fitness_score(c, q, np.eye(4, dtype=np.float32))
    tab, b = e.cloud_seed_grid(c)
    c.close(), q.close()
    e.close()
    return tab, b


def check_seed_tables():
    s = scene()
    e = make_engine()
    dev = {k: e.upload(s.clouds[k]) for k in SEED_CLOUDS}
    eye = np.eye(4, dtype=np.float32)
    for c in dev.values():
        tab, b = e.cloud_seed_grid(c)
        assert len(tab) == 0 and b == 0
    # k1 already has a grid when the batch arrives
    e.calc_fitness_score(dev["k1"], dev["q63"], eye)
    before, before_bits = e.cloud_seed_grid(dev["k1"])
    assert len(before) > 0
    pairs = [(dev[a], dev[SEED_CLOUDS[(i + 1) % len(SEED_CLOUDS)]], eye) for i, a in enumerate(SEED_CLOUDS)]
    e.calc_fitness_scores(pairs)
    bits_seen = set()
    for name in SEED_CLOUDS:
        tab, b = e.cloud_seed_grid(dev[name])
        ref, ref_b = _single_build_table(name)
        assert b == ref_b and len(tab) == len(ref) == (1 << b) + (1 << (b - 2)) + (1 << (b - 4)), (name, b, ref_b, len(tab), len(ref))
        diff = np.flatnonzero(tab != ref)
        assert diff.size == 0, (name, diff.size, diff[:8], tab[diff[:8]], ref[diff[:8]])
        n = len(s.clouds[name])
        filled = tab[tab != 0xffffffff]
        assert 0 < filled.size and filled.max() < n, (name, filled.size, n)
        bits_seen.add(b)
    assert len(bits_seen) >= 2, bits_seen                          # tables of different sizes in one launch
    after, after_bits = e.cloud_seed_grid(dev["k1"])
    assert after_bits == before_bits and (after == before).all()
    for c in dev.values():
        c.close()
    e.close()
    # seed_grid = 0: the batch builds none
    e = make_engine(seed_grid=0)
    dev = {k: e.upload(s.clouds[k]) for k in SEED_CLOUDS}
    e.calc_fitness_scores([(dev[a], dev[SEED_CLOUDS[(i + 1) % len(SEED_CLOUDS)]], eye) for i, a in enumerate(SEED_CLOUDS)])
    for c in dev.values():
        tab, b = e.cloud_seed_grid(c)
        assert len(tab) == 0 and b == 0
        c.close()
    e.close()


# ------------------------------------------------------------------------------------------------ 4: handle state
def check_handle_state(method):
    """The batch neither reads nor changes the handle's own target and source."""
    s = scene()
    guess = s.relposes[2]

    def run(with_batch):
        case = Case(method)
        case.e.setInputTarget(case.dev["k2"])
        case.e.setInputSource(case.dev["k1"])
        first = case.e.align(guess)
        if with_batch:
            case.e.calc_fitness_scores(case.pairs([0, 3, 4, 12, 14]), 4.0)
        fit = case.e.getFitnessScore(4.0)
        n = case.e.last_num_inliers
        second = case.e.align(guess)
        out = (bytes(first), fit, n, bytes(second))
        case.close()
        return out

    a, b = run(False), run(True)
    assert a[0] == b[0] and bits(a[1]) == bits(b[1]) and a[2] == b[2] and a[3] == b[3], (a[1], b[1], a[2], b[2])
    assert a[2] > 0


# ------------------------------------------------------------------------------------------------ 5: refusals
def _raw(e, c1, c2, poses, n, scores, inliers):
    vp = C.c_void_p

    def ptrs(cs):
        return None if cs is None else (vp * max(len(cs), 1))(*[(c._h if c is not None else None) for c in cs])
    return L.lib().hgs_calc_fitness_score_batch(e._h, ptrs(c1), ptrs(c2), None if poses is None else poses.ctypes.data_as(vp), n, 4.0,
                                                None if scores is None else scores.ctypes.data_as(vp), None if inliers is None else inliers.ctypes.data_as(vp))


def check_refusals():
    """Every refused call returns HGS_ERR_INVALID_ARGUMENT with the output arrays untouched; the valid call behind it gives the first valid call's bits."""
    s = scene()
    e, other, gone = make_engine(), make_engine(), make_engine()
    a, b, foreign, orphan = e.upload(s.clouds["k0"]), e.upload(s.clouds["k1"]), other.upload(s.clouds["k0"]), gone.upload(s.clouds["k0"])
    gone.close()                       # `orphan` has outlived its engine
    poses = np.ascontiguousarray(np.stack([L.colmajor16(s.relposes[1])] * 2))

    def valid():
        sc, n = np.zeros(2), np.zeros(2, np.uint32)
        assert _raw(e, [a, b], [b, a], poses, 2, sc, n) == L.HGS_OK
        return bits(sc), n.tobytes()

    want = valid()
    assert want[0] != bits(np.zeros(2))
    refused = {
        "cloud1 NULL": lambda sc, n: _raw(e, None, [b, a], poses, 2, sc, n),
        "cloud2 NULL": lambda sc, n: _raw(e, [a, b], None, poses, 2, sc, n),
        "relposes NULL": lambda sc, n: _raw(e, [a, b], [b, a], None, 2, sc, n),
        "a NULL entry of cloud1": lambda sc, n: _raw(e, [a, None], [b, a], poses, 2, sc, n),
        "a NULL entry of cloud2": lambda sc, n: _raw(e, [a, b], [b, None], poses, 2, sc, n),
        "a cloud of another handle as a tree": lambda sc, n: _raw(e, [a, foreign], [b, a], poses, 2, sc, n),
        "a cloud of another handle as a query": lambda sc, n: _raw(e, [a, b], [foreign, a], poses, 2, sc, n),
        "an orphaned cloud": lambda sc, n: _raw(e, [a, b], [b, orphan], poses, 2, sc, n),
    }
    for what, call in refused.items():
        sc, n = np.full(2, -7.25), np.full(2, 0xabcdef01, np.uint32)
        assert call(sc, n) == L.HGS_ERR_INVALID_ARGUMENT, what
        assert (sc == -7.25).all() and (n == 0xabcdef01).all(), what
        assert valid() == want, what
    n = np.full(2, 0xabcdef01, np.uint32)
    assert _raw(e, [a, b], [b, a], poses, 2, None, n) == L.HGS_ERR_INVALID_ARGUMENT and (n == 0xabcdef01).all()       # scores NULL
    # num_inliers may be NULL; no pairs at all is fine, with or without arrays
    sc = np.zeros(2)
    assert _raw(e, [a, b], [b, a], poses, 2, sc, None) == L.HGS_OK and bits(sc) == want[0]
    sc = np.full(2, -7.25)
    assert _raw(e, None, None, None, 0, None, None) == L.HGS_OK and _raw(e, [a], [b], poses, 0, sc, None) == L.HGS_OK and (sc == -7.25).all()
    assert len(e.calc_fitness_scores([])) == 0
    assert valid() == want
    for c in (a, b, foreign, orphan):
        c.close()
    e.close(), other.close()


# ------------------------------------------------------------------------------------------------ 6: chunking
def check_chunking():
    which = [0, 1, 2, 3, 8, 11, 13, 14]
    case = Case()
    whole = case.e.calc_fitness_scores(case.pairs(which), 4.0, return_inliers=True)
    case.e.set_option("pair_chunk", 3)          # 3 + 3 + 2
    chunked = case.e.calc_fitness_scores(case.pairs(which), 4.0, return_inliers=True)
    case.close()
    fresh = Case()                              # ... and on an engine that builds everything inside the chunked call
    fresh.e.set_option("pair_chunk", 3)
    cold = fresh.e.calc_fitness_scores(fresh.pairs(which), 4.0, return_inliers=True)
    fresh.close()
    ref = reference("FAST_GICP", 1, 4.0)
    assert bits(whole[0]) == bits([ref[i][0] for i in which]) and list(whole[1]) == [ref[i][1] for i in which]
    for got in (chunked, cold):
        assert bits(got[0]) == bits(whole[0]) and (got[1] == whole[1]).all(), (got, whole)


# ------------------------------------------------------------------------------------------------ 7: information matrices
def check_information_matrices():
    import make_refpin_golden as MG
    gold = np.load(GOLDEN)
    c = MG.small_clouds()[0]
    reg = make_engine()
    d1, d2 = reg.upload(c["pair_target"]), reg.upload(c["pair_source"])
    calls = {"batch": 0, "single": 0}
    batch, single = reg.calc_fitness_scores, reg.calc_fitness_score

    def count(name, f):
        def g(*a, **kw):
            calls[name] += 1
            return f(*a, **kw)
        return g
    reg.calc_fitness_scores, reg.calc_fitness_score = count("batch", batch), count("single", single)
    by_params = {}
    for i, prm in enumerate(gold["inf_params"]):
        by_params.setdefault(str(prm), []).append(i)
    assert len(by_params) >= 3 and sum(len(v) for v in by_params.values()) == len(gold["inf_matrix"])
    for prm, rows in by_params.items():
        calc = InformationMatrixCalculator(json.loads(prm))
        edges = [(d1, d2, gold["fit_pose"][int(gold["inf_pose_case"][i])]) for i in rows]
        before = dict(calls)
        mats = calc.calc_information_matrices(reg, edges)
        if calc.use_const_inf_matrix:
            assert calls == before, prm                                    # no device call
        else:
            assert calls["batch"] == before["batch"] + 1 and calls["single"] == before["single"], prm
        assert len(mats) == len(rows)
        for M, i, edge in zip(mats, rows, edges):
            one = calc.calc_information_matrix(reg, *edge)
            assert M.tobytes() == one.tobytes(), (prm, i)
            assert np.allclose(M, gold["inf_matrix"][i], rtol=1e-5, atol=0), (prm, i)      # d(weight)/d(score) amplifies the 4e-7 of the score
    d1.close(), d2.close()
    reg.close()


# ------------------------------------------------------------------------------------------------ 8: the C++ adapter
def write_cpp_inputs(tmp_path):
    """The scene as files for tests/cpp/edge_fitness_main.cpp; returns its arguments."""
    s = scene()
    ids = {k: i for i, k in enumerate(s.clouds)}
    args = ["4.0", str(tmp_path / "poses.bin")]
    for k, c in s.clouds.items():
        c.tofile(tmp_path / f"{k}.bin")
        args.append(f"C:{ids[k]}:{tmp_path / (k + '.bin')}")
    args += [f"P:{ids[a]}:{ids[b]}" for a, b in s.pairs]
    np.stack([L.colmajor16(T) for T in s.relposes]).astype(np.float32).tofile(tmp_path / "poses.bin")
    return args


def check_cpp_output(lines):
    """edge_fitness_main prints the scores of fitness_scores ("B") and of fitness_score per pair ("S") as hex doubles: the same strings."""
    assert lines[-1].startswith("mismatches 0"), lines[-1]
    batch = [l.split()[1:] for l in lines if l.startswith("B ")]
    single = [l.split()[1:] for l in lines if l.startswith("S ")]
    n = len(scene().pairs)
    assert len(batch) == len(single) == n and batch == single, (batch, single)
    ref = reference("FAST_GICP", 1, 4.0)
    assert [float.fromhex(b[1]) for b in batch] == [r[0] for r in ref]
    assert any(l.startswith("device_calls batch 1") for l in lines), lines[-3:]


# ------------------------------------------------------------------------------------------------ 9: allocation accounting (emulation)
def live_objects():
    """{memory blocks, streams, events} the emulated HIP runtime has handed out and not taken back (tests/emul/simt_runtime.cpp)."""
    out = (C.c_longlong * 3)()
    L.lib().simt_read_live_objects(out)
    return tuple(out)


def check_allocation():
    """Batched calls (cold, chunked, cached), an invalidated cloud, then hgs_destroy: nothing stays allocated."""
    before = live_objects()
    for method in METHODS:
        case = Case(method)
        which = [1, 2, 3, 8, 12, 14]
        a = case.e.calc_fitness_scores(case.pairs(which), 4.0)
        size = case.dev["k1"].device_bytes
        case.dev["k1"].invalidate()
        case.e.set_option("pair_chunk", 2)
        b = case.e.calc_fitness_scores(case.pairs(which), 4.0)
        assert bits(a) == bits(b) and case.dev["k1"].device_bytes == size > 0
        case.close()
    assert live_objects() == before
