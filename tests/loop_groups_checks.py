"""Shared checks of hgs_loop_match_groups — the candidates of several new keyframes in one device batch (LoopDetector::detect,
loop_detector.hpp:57-68) — run on an MI355X (tests/test_loop_groups_gpu.py) and on the same kernels emulated on the host
(tests/test_loop_groups_simt_host.py).  The yardstick is exact: a problem's record depends on its own target, source and guess only, so
every record of the grouped call equals, bit for bit, what hgs_set_target_cloud + hgs_loop_match_batch over its group alone give on a
fresh engine."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from hdl_graph_slam_amd import _lib as L, synth, workloads
from hdl_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
from hdl_graph_slam_amd.registration import RegistrationHIP

METHODS = {"FAST_GICP": (L.HGS_FAST_GICP, False), "ICP_HIP": (L.HGS_ICP, False), "ICP_HIP_reciprocal": (L.HGS_ICP, True)}

# engine options of the grouped engine (hgs_debug_set_option); every variant sets all of them, so one engine serves them in any order.
# 9 small problems run on one lane and in two-launch rounds by default: "lanes4" cuts them 2 | 2 | 2 | 3, i.e. inside the second and the
# last group; the others select the remaining instantiations of k_gicp_linearize / k_gicp_error.
_BASE = {"batch_lanes": 0, "fused_rounds": 1, "fused_rounds_max_problems": 4, "fused_rounds_max_blocks": 640, "nn_qpw": 0}
_ROUND2 = {"fused_rounds": 1, "fused_rounds_max_problems": 64, "fused_rounds_max_blocks": 1 << 20}
VARIANTS = {
    "default": {},
    "lanes4": {"batch_lanes": 4},
    "two_launch_on": _ROUND2,
    "two_launch_off": {"fused_rounds": 0},
    "nn_qpw16": dict(_ROUND2, nn_qpw=16),
    "nn_qpw32": dict(_ROUND2, nn_qpw=32),
    "nn_qpw64": dict(_ROUND2, nn_qpw=64),
}
GICP_VARIANTS = list(VARIANTS)
ICP_VARIANTS = ["default", "lanes4"]      # (the other options only reach FAST_GICP's kernels)


def params(name):
    method, reciprocal = METHODS[name]
    p = L.default_params(method)
    p.use_reciprocal_correspondences = reciprocal
    return p


def make_engine(p):
    return RegistrationHIP(p)


class Scene:
    """Three targets of ~9 000, ~2 500 and ~700 points cut from one scan (their trees are 2048, 512 and 128 leaves deep), four candidate
    scans, one with non-finite rows, one empty; groups of 1, 3, 0 and 5 candidates = 9 problems.  c0 and c1 are candidates of two groups;
    B is the target of the second group and a candidate of the last."""

    def __init__(self):
        wl = workloads.make_loop_closure_set("HDL-32E", 3, n_candidates=4, n_distinct=4, downsample=0.5, spread=6.0, guess_noise=(0.3, 1.0))
        A = workloads.make_loop_closure_set("HDL-32E", 3, n_candidates=1, n_distinct=1, downsample=0.26, spread=6.0).target
        self.clouds = {"A": A, "B": np.ascontiguousarray(A[1::4][:2500]), "C": np.ascontiguousarray(A[2::13][:700])}
        for i, c in enumerate(wl.candidates):
            self.clouds[f"c{i}"] = c
        bad = wl.candidates[3].copy()
        bad["x"][[5, 100, len(bad) - 1]] = np.nan
        bad["y"][[7, 640]] = np.inf
        bad["z"][1000] = -np.inf
        self.clouds["nan"] = bad
        self.clouds["empty"] = wl.candidates[0][:0].copy()
        drift = synth.pose_matrix([0.2, -0.1, 0.0], [0.0, 0.0, 0.02]).astype(np.float32)    # odometry-like: decimetres, a degree
        g = {f"c{i}": wl.guesses[i] for i in range(4)}
        g.update(nan=wl.guesses[3], B=drift, empty=np.eye(4, dtype=np.float32))
        self.targets = ["A", "B", None, "C"]
        self.groups = [["c0"], ["c1", "nan", "c0"], [], ["c2", "B", "empty", "c3", "c1"]]
        self.guesses = [[g[c] for c in grp] for grp in self.groups]


@functools.lru_cache(maxsize=None)
def scene() -> Scene:
    return Scene()


class Case:
    """One engine of a method with the scene's clouds resident."""

    def __init__(self, name, engine_factory=make_engine):
        self.name = name
        self.e = engine_factory(params(name))
        self.dev = {k: self.e.upload(v) for k, v in scene().clouds.items()}

    def grouped(self, **kw):
        s = scene()
        return self.e.loop_match_groups([self.dev[t] if t else None for t in s.targets], [[self.dev[c] for c in g] for g in s.groups], s.guesses, 4.0, **kw)

    def close(self):
        for c in self.dev.values():
            c.close()
        self.e.close()


_reference = {}


def reference(name, engine_factory=make_engine):
    """[(records, best) or None per group] of one hgs_loop_match_batch per non-empty group on a fresh engine (default options); computed
    once per method and library."""
    key = (L.LIB_PATH, name)
    if key not in _reference:
        case = Case(name, engine_factory)
        s = scene()
        out = []
        for t, grp, gs in zip(s.targets, s.groups, s.guesses):
            if not grp:
                out.append(None)
                continue
            case.e.setInputTarget(case.dev[t])
            out.append(case.e.loop_match_batch([case.dev[c] for c in grp], gs, 4.0))
        case.close()
        _reference[key] = out
    return _reference[key]


def assert_records_equal(rec, ref, where):
    assert len(rec) == len(ref), where
    if rec.tobytes() == ref.tobytes():
        return
    for i in range(len(rec)):
        for f in L.RESULT_DTYPE.names:
            assert np.asarray(rec[i][f]).tobytes() == np.asarray(ref[i][f]).tobytes(), (where, i, f, rec[i][f], ref[i][f])


def check_records(case: Case, variant, engine_factory=make_engine):
    """Every field of every record, and best per group, against the per-target batches."""
    for k, v in dict(_BASE, **VARIANTS[variant]).items():
        case.e.set_option(k, v)
    rec, best = case.grouped()
    ref = reference(case.name, engine_factory)
    s = scene()
    assert len(rec) == sum(len(g) for g in s.groups) == 9
    first = 0
    for g, grp in enumerate(s.groups):
        if not grp:
            assert best[g] == -1
            continue
        assert_records_equal(rec[first:first + len(grp)], ref[g][0], (case.name, variant, g))
        assert best[g] == ref[g][1], (case.name, variant, g, best[g], ref[g][1])
        assert list(rec["candidate_id"][first:first + len(grp)]) == list(range(len(grp)))
        first += len(grp)
    # the check is about something: most registrations converge after some iterations, every non-empty group has a winner
    assert rec["converged"].sum() >= 6 and (rec["iterations"] >= 1).sum() >= 6 and all(best[g] >= 0 for g in (0, 1, 3)), (rec["converged"], rec["iterations"], best)
    return rec, best


def check_handle_state(case: Case):
    """The grouped call neither uses nor changes the handle's own target and source."""
    s = scene()
    case.e.setInputTarget(case.dev["B"])
    case.e.setInputSource(case.dev["c2"])
    g = s.guesses[3][0]
    before = case.e.align(g)
    before_fit = case.e.getFitnessScore(4.0)
    case.grouped()
    after = case.e.align(g)
    assert bytes(before) == bytes(after)
    assert case.e.getFitnessScore(4.0) == before_fit
    # ... and without any target or source set it runs just the same
    fresh = Case(case.name)
    rec, best = fresh.grouped()
    rec0, best0 = case.grouped()
    assert rec.tobytes() == rec0.tobytes() and list(best) == list(best0)
    fresh.close()


def _raw_groups(e, targets, offsets, cands, guesses):
    off = np.asarray(offsets, np.uintp)
    n = len(cands)
    tptr = (C.c_void_p * max(len(targets), 1))(*[t._h if t is not None else None for t in targets])
    cptr = (C.c_void_p * max(n, 1))(*[c._h for c in cands])
    g = np.ascontiguousarray(np.stack([L.colmajor16(T) for T in guesses]))
    out = np.zeros(n, dtype=L.RESULT_DTYPE)
    best = np.full(len(targets), -1, np.int32)
    return L.lib().hgs_loop_match_groups(e._h, tptr, len(targets), off.ctypes.data_as(C.c_void_p), cptr, g.ctypes.data_as(C.c_void_p), 4.0,
                                         out.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p))


def check_refusals(engine_factory=make_engine):
    """Every refused call returns its status and leaves the engine usable: the valid call behind it gives the first valid call's records."""
    s = scene()
    small_t, small_a, small_b = s.clouds["C"], np.ascontiguousarray(s.clouds["c0"][::6]), np.ascontiguousarray(s.clouds["c1"][::6])
    eye = np.eye(4, dtype=np.float32)
    e, other = engine_factory(params("FAST_GICP")), engine_factory(params("FAST_GICP"))
    t, a, b, foreign = e.upload(small_t), e.upload(small_a), e.upload(small_b), other.upload(small_a)

    def valid():
        rec, best, rc = e.loop_match_groups([t, a], [[a, b], [b]], [[eye, eye], [eye]], 4.0, return_status=True)
        assert rc == L.HGS_OK
        return rec.tobytes(), list(best)

    want = valid()
    refused = {
        "a duplicate inside a group": lambda: e.loop_match_groups([t], [[a, a]], [[eye, eye]], 4.0, return_status=True)[2],
        "a foreign candidate": lambda: e.loop_match_groups([t], [[a, foreign]], [[eye, eye]], 4.0, return_status=True)[2],
        "a foreign target": lambda: e.loop_match_groups([foreign], [[a]], [[eye]], 4.0, return_status=True)[2],
        "a NULL target of a non-empty group": lambda: e.loop_match_groups([t, None], [[a], [b]], [[eye], [eye]], 4.0, return_status=True)[2],
        "offsets that decrease": lambda: _raw_groups(e, [t, t], [0, 2, 1], [a, b], [eye, eye]),
        "offsets that do not start at 0": lambda: _raw_groups(e, [t], [1, 2], [a, b], [eye, eye]),
    }
    for what, call in refused.items():
        assert call() == L.HGS_ERR_INVALID_ARGUMENT, what
        assert valid() == want, what
    # the same cloud in two groups, and as target and candidate, is the normal case (covered by `valid`); no groups at all is fine
    assert e.loop_match_groups([], [], [], 4.0, return_status=True)[2] == L.HGS_OK
    assert e.loop_match_groups([None], [[]], [[]], 4.0, return_status=True)[2] == L.HGS_OK
    for c in (t, a, b, foreign):
        c.close()
    e.close(), other.close()
    for method in (L.HGS_NDT_OMP, L.HGS_FAST_VGICP):
        p = L.default_params(method)
        p.resolution = 1.0
        e = engine_factory(p)
        t, a = e.upload(small_t), e.upload(small_a)
        assert e.loop_match_groups([t], [[a]], [[eye]], 4.0, return_status=True)[2] == L.HGS_ERR_UNSUPPORTED
        e.setInputTarget(t)
        rec, _ = e.loop_match_batch([a], [eye], 4.0)
        assert len(rec) == 1 and rec["candidate_id"][0] == 0 and np.isfinite(rec["final_transformation"]).all()
        t.close(), a.close()
        e.close()


# ------------------------------------------------------------------------------------------------ LoopDetector.detect
def _detect_scene(n_old, new_specs, leaf):
    """Keyframes along the corridor of one synthetic scene: n_old old ones a metre apart, the new ones at (x, accum_distance); every estimate is
    the true pose with a little drift on it."""
    sc = synth.make_scene(5)
    rng = np.random.default_rng(11)

    def frame(x, accum, seed):
        pose = synth.pose_matrix([x, 0.1 * np.sin(x), 0.0], [0.0, 0.0, 0.03 * x])
        cloud = synth.voxel_downsample(synth.scan(sc, "VLP-16", pose, seed), leaf)
        est = pose @ synth.pose_matrix(rng.normal(0, 0.05, 3) * [1, 1, 0], [0.0, 0.0, rng.normal(0, 0.005)])
        return cloud, est, float(accum)

    old = [frame(-0.5 * (n_old - 1) + i, i, 100 + i) for i in range(n_old)]
    new = [frame(x, accum, 200 + i) for i, (x, accum) in enumerate(new_specs)]
    return old, new


def _run_detect(pnh, old, new, last_edge):
    ld = LoopDetector(pnh)
    calls = {"groups": 0, "batch": 0}
    reg = ld.registration
    groups, batch = reg.loop_match_groups, reg.loop_match_batch

    def count(name, f):
        def g(*a, **kw):
            calls[name] += 1
            return f(*a, **kw)
        return g
    reg.loop_match_groups, reg.loop_match_batch = count("groups", groups), count("batch", batch)
    ld.last_edge_accum_distance = last_edge
    kfs = [KeyFrame(c, e, a, id=i) for i, (c, e, a) in enumerate(old)]
    nks = [KeyFrame(c, e, a, id=len(old) + i) for i, (c, e, a) in enumerate(new)]
    loops = ld.detect(kfs, nks)
    out = [(nks.index(l.key1), kfs.index(l.key2), l.relative_pose.tobytes()) for l in loops]
    result = (out, ld.last_edge_accum_distance, ld.last_detect_grouped, dict(calls))
    reg.close()
    return result


def check_detect(method="FAST_GICP"):
    """reg_hip_batch_new_keyframes: the loops, their order, their relative poses (bitwise) and the final last_edge_accum_distance equal the
    sequential detect.  Five new keyframes over eight old ones, last loop edge at 100 m, min_edge_interval 5 m: the first (103 m) fails the
    gate at entry; the second (110 m) finds a loop; the third (112 m) passed the gate at entry, is matched speculatively and discarded in the
    replay; the fourth and fifth (120 m, 126 m) pass again."""
    pnh = {"registration_method": method, "fitness_score_thresh": 2.5, "fitness_score_max_range": 4.0, "distance_thresh": 1.6,
           "accum_distance_thresh": 8.0, "min_edge_interval": 5.0}
    old, new = _detect_scene(8, [(-1.0, 103.0), (0.0, 110.0), (0.5, 112.0), (1.5, 120.0), (2.5, 126.0)], 1.0)
    seq = _run_detect(pnh, old, new, 100.0)
    grp = _run_detect(dict(pnh, reg_hip_batch_new_keyframes=True), old, new, 100.0)
    assert seq[0] == grp[0] and seq[1] == grp[1], (seq[0], grp[0], seq[1], grp[1])
    found = [l[0] for l in seq[0]]
    assert 1 in found and 3 in found and 0 not in found and 2 not in found, found
    assert not seq[2] and seq[3] == {"groups": 0, "batch": len(found)}          # with the key off: today's calls
    assert grp[2] and grp[3] == {"groups": 1, "batch": 0}


def check_detect_falls_back(method="NDT_OMP"):
    """An engine that does not serve the grouped call: the key changes nothing."""
    pnh = {"registration_method": method, "reg_resolution": 1.0, "fitness_score_thresh": 2.5, "fitness_score_max_range": 4.0, "distance_thresh": 1.1,
           "accum_distance_thresh": 8.0, "min_edge_interval": 5.0}
    old, new = _detect_scene(3, [(0.0, 110.0), (1.0, 120.0)], 1.2)
    seq = _run_detect(pnh, old, new, 100.0)
    grp = _run_detect(dict(pnh, reg_hip_batch_new_keyframes=True), old, new, 100.0)
    assert seq[:3] == grp[:3] and not grp[2]
    assert grp[3]["batch"] == seq[3]["batch"] == 2 and grp[3]["groups"] == 1      # asked once, answered HGS_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the C++ matcher
def write_cpp_inputs(tmp_path):
    """The scene's non-empty groups as files for tests/cpp/loop_groups_main.cpp; returns its arguments behind the engine count."""
    s = scene()
    ids = {k: i for i, k in enumerate(s.clouds)}
    for k, c in s.clouds.items():
        c.tofile(tmp_path / f"{k}.bin")
    args, guesses = [], []
    for t, grp, gs in zip(s.targets, s.groups, s.guesses):
        if not grp:
            continue
        args.append(f"T:{ids[t]}:{tmp_path / (t + '.bin')}")
        for c, g in zip(grp, gs):
            args.append(f"C:{ids[c]}:{tmp_path / (c + '.bin')}")
            guesses.append(L.colmajor16(g))
    np.stack(guesses).astype(np.float32).tofile(tmp_path / "guesses.bin")
    return ["4.0", str(tmp_path / "guesses.bin"), *args]


def check_cpp_output(lines):
    """loop_groups_main prints the records of match_groups and then of match per group, as hex: equal line by line."""
    assert lines[-1].startswith("mismatches 0"), lines[-1]
    grouped = [l for l in lines if l.startswith("G ")]
    single = [l for l in lines if l.startswith("S ")]
    assert len(grouped) == len(single) == 9 + 3                    # 9 records + 3 "best" lines
    assert [l[2:] for l in grouped] == [l[2:] for l in single]
    assert any(l.split()[1] == "best" and int(l.split()[3]) >= 0 for l in grouped)


def live_objects():
    """{memory blocks, streams, events} the emulated HIP runtime has handed out and not taken back (tests/emul/simt_runtime.cpp)."""
    out = (C.c_longlong * 3)()
    L.lib().simt_read_live_objects(out)
    return tuple(out)


def check_allocation(engine_factory=make_engine):
    """A grouped call on several lanes, then hgs_destroy: nothing stays allocated."""
    s = scene()
    before = live_objects()
    eye = np.eye(4, dtype=np.float32)
    for name in ("FAST_GICP", "ICP_HIP"):
        e = engine_factory(params(name))
        e.set_option("batch_lanes", 4)
        t, a, b = e.upload(s.clouds["C"]), e.upload(np.ascontiguousarray(s.clouds["c0"][::6])), e.upload(np.ascontiguousarray(s.clouds["c1"][::6]))
        rec, best = e.loop_match_groups([t, a, b], [[a, b], [b, t], [t]], [[eye, eye], [eye, eye], [eye]], 4.0)
        assert len(rec) == 5
        for c in (t, a, b):
            c.close()
        e.close()
    assert live_objects() == before
