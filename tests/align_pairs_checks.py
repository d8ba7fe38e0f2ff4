"""Shared checks of hgs_align_pairs — n independent registrations (target i, source i, guess i) in one device batch, every engine — run on an
MI355X (tests/test_align_pairs_gpu.py) and on the same kernels emulated on the host (tests/test_align_pairs_simt_host.py).  The yardstick is
exact: a problem's record depends on its own target, source and guess only, so every record of the paired call equals, bit for bit, what
hgs_set_target_cloud + hgs_loop_match_batch over that one source give on a fresh engine."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import loop_groups_checks as GC
from hdl_graph_slam_amd import _lib as L, synth
from hdl_graph_slam_amd.loop_detector import KeyFrame, LoopDetector
from hdl_graph_slam_amd.odometry import LockstepOdometry, ScanMatchingOdometry
from hdl_graph_slam_amd.registration import RegistrationHIP

MAX_RANGE = 4.0


def _params(method, resolution=None, search=None, reciprocal=False):
    def make():
        p = L.default_params(method)
        p.use_reciprocal_correspondences = reciprocal
        if resolution is not None:
            p.resolution = resolution
        if search is not None:
            p.neighbor_search = search
        return p
    return make


METHODS = {
    "FAST_GICP": _params(L.HGS_FAST_GICP),
    "ICP_HIP": _params(L.HGS_ICP),
    "ICP_HIP_reciprocal": _params(L.HGS_ICP, reciprocal=True),
    "FAST_VGICP_DIRECT1": _params(L.HGS_FAST_VGICP, 1.0, L.HGS_DIRECT1),
    "FAST_VGICP_DIRECT7": _params(L.HGS_FAST_VGICP, 1.0, L.HGS_DIRECT7),
    "FAST_VGICP_DIRECT27": _params(L.HGS_FAST_VGICP, 1.0, L.HGS_DIRECT27),
    "NDT_OMP_DIRECT1": _params(L.HGS_NDT_OMP, 1.0, L.HGS_DIRECT1),
    "NDT_OMP_DIRECT7": _params(L.HGS_NDT_OMP, 1.0, L.HGS_DIRECT7),
    "NDT_OMP_KDTREE": _params(L.HGS_NDT_OMP, 1.0, L.HGS_KDTREE),
}

# The clouds of loop_groups_checks.scene() as ten pairs (target, source):
#   * consecutive problems have different targets; A serves the non-adjacent problems 0, 3, 6 and 9;
#   * c0 is a source three times; B is a target (1, 4, 8) and a source (6); problem 5 registers c2 against itself;
#   * the source with non-finite rows (3) and the empty source (7) are in; C (~700 points: few or no valid NDT cells at resolution 1.0) is a target twice.
PAIRS = [("A", "c0"), ("B", "c1"), ("C", "c2"), ("A", "nan"), ("B", "c0"), ("c2", "c2"), ("A", "B"), ("C", "empty"), ("B", "c3"), ("A", "c2")]
ALIGN_PAIRS = (0, 4, 6)      # check 3: the pairs compared with hgs_set_target_cloud + hgs_set_source_cloud + hgs_align


# The scene's guesses are loop-closure guesses (noise 0.3 m / 1 degree).  ICP with reciprocal correspondences settles from them in one or two
# iterations, which would make its reference records trivial (reference() asserts that they are not): its guesses carry this much more.
GUESS_NOISE = {"ICP_HIP_reciprocal": synth.pose_matrix([0.6, -0.5, 0.0], [0.0, 0.0, 0.05]).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def _guesses(name):
    s = GC.scene()
    g = {c: gg for grp, gs in zip(s.groups, s.guesses) for c, gg in zip(grp, gs)}           # the scene's guess of every cloud against A / B / C
    drift = g["B"]
    noise = GUESS_NOISE.get(name, np.eye(4, dtype=np.float32))
    return [(np.asarray(drift if t == src else g[src], np.float32) @ noise).astype(np.float32) for t, src in PAIRS]


def guesses(name):
    return list(_guesses(name))


# engine options of the paired engine (hgs_debug_set_option); every variant sets all of its method's keys, so one engine serves them in any order
_BASE_ALL = {"batch_lanes": 0}
_BASE_NDT = {"ndt_resident": 0, "ndt_chunk": 0, "ndt_sort": -1}
_LANES4 = {"batch_lanes": 4}                      # 10 problems cut 2 | 2 | 3 | 3: every cut falls between problems with different targets
NDT_VARIANTS = {
    "default": {},
    "lanes4": _LANES4,
    # with the default block count a batch this small gives every block one static item and no block ever changes problem; with one or two
    # resident blocks a block's run crosses several problems and targets — the reload path of k_ndt_pass's per-problem form
    "resident1_chunk8": {"ndt_resident": 1, "ndt_chunk": 8},
    "resident1_chunk2": {"ndt_resident": 1, "ndt_chunk": 2},
    "resident2_chunk8": {"ndt_resident": 2, "ndt_chunk": 8},
    "resident2_chunk2": {"ndt_resident": 2, "ndt_chunk": 2},
    "resident2_chunk2_lanes4": {"ndt_resident": 2, "ndt_chunk": 2, "batch_lanes": 4},
    "sort0": {"ndt_sort": 0, "ndt_resident": 2, "ndt_chunk": 8},
    "sort1": {"ndt_sort": 1, "ndt_resident": 2, "ndt_chunk": 8},
}
VGICP_VARIANTS = {"default": {}, "lanes4": _LANES4}
ICP_VARIANTS = {"default": {}, "lanes4": _LANES4}
GICP_VARIANTS = GC.VARIANTS


def variants_of(name):
    if name.startswith("NDT"):
        return NDT_VARIANTS, dict(_BASE_ALL, **_BASE_NDT)
    if name.startswith("FAST_VGICP"):
        return VGICP_VARIANTS, _BASE_ALL
    if name == "FAST_GICP":
        return GICP_VARIANTS, GC._BASE
    return ICP_VARIANTS, _BASE_ALL


class Case:
    """One engine of a method with the scene's clouds resident."""

    def __init__(self, name):
        self.name = name
        self.e = RegistrationHIP(METHODS[name]())
        self.dev = {k: self.e.upload(v) for k, v in GC.scene().clouds.items()}

    def paired(self, max_range=MAX_RANGE, pairs=None, **kw):
        idx = range(len(PAIRS)) if pairs is None else pairs
        g = guesses(self.name)
        return self.e.align_pairs([self.dev[PAIRS[i][0]] for i in idx], [self.dev[PAIRS[i][1]] for i in idx], [g[i] for i in idx], max_range, **kw)

    def close(self):
        for c in self.dev.values():
            c.close()
        self.e.close()


_reference = {}


def reference(name):
    """The records of hgs_set_target_cloud(target i) + hgs_loop_match_batch({source i}, guess i, 4.0), pair after pair, on a fresh engine with default
    options; computed once per method and library."""
    key = (L.LIB_PATH, name)
    if key not in _reference:
        case = Case(name)
        out = np.zeros(len(PAIRS), dtype=L.RESULT_DTYPE)
        for i, ((t, s), g) in enumerate(zip(PAIRS, guesses(name))):
            case.e.setInputTarget(case.dev[t])
            rec, _ = case.e.loop_match_batch([case.dev[s]], [g], MAX_RANGE)
            out[i] = rec[0]
        case.close()
        # the scene is not trivial for this engine: at least 6 problems run two or more iterations and end away from their guess
        moved = [not np.array_equal(out["final_transformation"][i], L.colmajor16(g)) for i, g in enumerate(guesses(name))]
        busy = sum(1 for i in range(len(PAIRS)) if out["iterations"][i] >= 2 and moved[i])
        assert busy >= 6, (name, out["iterations"], moved)
        out.setflags(write=False)
        _reference[key] = out
    return _reference[key]


_REG_FIELDS = [f for f in L.RESULT_DTYPE.names if f not in ("fitness_score", "num_inliers", "candidate_id")]


def assert_pairs_equal(rec, ref, where, idx=None, with_fitness=True):
    idx = list(range(len(ref))) if idx is None else list(idx)
    assert len(rec) == len(idx), where
    for k, i in enumerate(idx):
        assert rec["candidate_id"][k] == k, (where, k)
        for f in _REG_FIELDS + (["fitness_score", "num_inliers"] if with_fitness else []):
            assert np.asarray(rec[k][f]).tobytes() == np.asarray(ref[i][f]).tobytes(), (where, i, f, rec[k][f], ref[i][f])
        if not with_fitness:
            assert np.isnan(rec["fitness_score"][k]) and rec["num_inliers"][k] == 0, (where, i)


def set_variant(case: Case, variant):
    variants, base = variants_of(case.name)
    for k, v in dict(base, **variants[variant]).items():
        case.e.set_option(k, v)


def check_records(case: Case, variant="default"):
    """Checks 1 and 2: every field of every record against the yardstick, with and without the fitness pass."""
    set_variant(case, variant)
    ref = reference(case.name)
    assert_pairs_equal(case.paired(), ref, (case.name, variant, "fitness"))
    assert_pairs_equal(case.paired(max_range=None), ref, (case.name, variant, "no fitness"), with_fitness=False)
    set_variant(case, "default")


def check_align_agreement(case: Case):
    """Check 3: three pairs against hgs_set_target_cloud + hgs_set_source_cloud + hgs_align on a fresh engine."""
    rec = case.paired(max_range=None, pairs=ALIGN_PAIRS)
    assert_pairs_equal(rec, reference(case.name), (case.name, "pairs subset"), idx=ALIGN_PAIRS, with_fitness=False)
    fresh = Case(case.name)
    g = guesses(case.name)
    for k, i in enumerate(ALIGN_PAIRS):
        fresh.e.setInputTarget(fresh.dev[PAIRS[i][0]])
        fresh.e.setInputSource(fresh.dev[PAIRS[i][1]])
        r = fresh.e.align(g[i])
        got = (rec["final_transformation"][k].tobytes(), int(rec["converged"][k]), int(rec["iterations"][k]), float(rec["error"][k]).hex(), int(rec["lm_tries"][k]))
        want = (bytes(r.final_transformation), r.converged, r.iterations, float(r.error).hex(), r.lm_tries)
        assert got == want, (case.name, i, got[1:], want[1:])
    fresh.close()


def check_handle_state(case: Case):
    """Check 4: the paired call neither uses nor changes the handle's own target and source; and it runs without either."""
    g = guesses(case.name)
    case.e.setInputTarget(case.dev["B"])
    case.e.setInputSource(case.dev["c2"])
    before = case.e.align(g[2])
    case.paired()
    case.paired(max_range=None, pairs=(0,))       # (one pair without a fitness pass: FAST_GICP hands it over as hgs_align's result is)
    after = case.e.align(g[2])
    assert bytes(before) == bytes(after)
    fresh = Case(case.name)
    assert_pairs_equal(fresh.paired(), reference(case.name), (case.name, "no target or source set"))
    fresh.close()


def check_shapes_back_to_back(case: Case):
    """Check 4, second half: a larger call, then a smaller one with other targets in front — no lane plan and no target view of the first survives."""
    ref = reference(case.name)
    for variant in ("default", "lanes4", "resident2_chunk2"):
        if variant not in variants_of(case.name)[0]:
            continue
        set_variant(case, variant)
        assert_pairs_equal(case.paired(), ref, (case.name, variant, "larger"))
        small = (8, 2, 5)
        assert_pairs_equal(case.paired(pairs=small), ref, (case.name, variant, "smaller"), idx=small)
    set_variant(case, "default")


def _raw_pairs(e, tptr, sptr, n, out_ptr, with_range=True):
    g = np.ascontiguousarray(np.stack([L.colmajor16(np.eye(4, dtype=np.float32))] * max(n, 1)))
    rng = C.byref(C.c_double(MAX_RANGE)) if with_range else None
    return L.lib().hgs_align_pairs(e._h, tptr, sptr, g.ctypes.data_as(C.c_void_p), rng, n, out_ptr)


def check_refusals():
    """Check 5: every refused call returns its status and leaves the engine usable: the valid call behind it gives the first valid call's records."""
    s = GC.scene()
    small_t, small_a, small_b = s.clouds["C"], np.ascontiguousarray(s.clouds["c0"][::6]), np.ascontiguousarray(s.clouds["c1"][::6])
    eye = np.eye(4, dtype=np.float32)
    for name in ("FAST_GICP", "NDT_OMP_DIRECT7", "FAST_VGICP_DIRECT7"):
        e, other = RegistrationHIP(METHODS[name]()), RegistrationHIP(METHODS[name]())
        t, a, b, foreign = e.upload(small_t), e.upload(small_a), e.upload(small_b), other.upload(small_a)

        def valid():
            rec, rc = e.align_pairs([t, a, t], [a, b, b], [eye, eye, eye], MAX_RANGE, return_status=True)
            assert rc == L.HGS_OK
            return rec.tobytes()

        want = valid()
        out = np.zeros(2, dtype=L.RESULT_DTYPE)
        two = lambda x, y: (C.c_void_p * 2)(x._h if x is not None else None, y._h if y is not None else None)
        refused = {
            "a NULL target": lambda: e.align_pairs([t, None], [a, b], [eye, eye], MAX_RANGE, return_status=True)[1],
            "a NULL source": lambda: e.align_pairs([t, t], [a, None], [eye, eye], MAX_RANGE, return_status=True)[1],
            "a foreign source": lambda: e.align_pairs([t, t], [a, foreign], [eye, eye], None, return_status=True)[1],
            "a foreign target": lambda: e.align_pairs([t, foreign], [a, b], [eye, eye], MAX_RANGE, return_status=True)[1],
            "NULL out with n > 0": lambda: _raw_pairs(e, two(t, t), two(a, b), 2, None),
            "NULL targets with n > 0": lambda: _raw_pairs(e, None, two(a, b), 2, out.ctypes.data_as(C.c_void_p)),
        }
        for what, call in refused.items():
            assert call() == L.HGS_ERR_INVALID_ARGUMENT, (name, what)
            assert valid() == want, (name, what)
        assert _raw_pairs(e, None, None, 0, None) == L.HGS_OK                       # no pairs at all is fine, whatever the pointers
        rec, rc = e.align_pairs([], [], [], MAX_RANGE, return_status=True)
        assert rc == L.HGS_OK and len(rec) == 0 and valid() == want
        for c in (t, a, b, foreign):
            c.close()
        e.close(), other.close()


def check_vgicp_oversized_grid(case: Case):
    """Check 5, FAST_VGICP: one pair whose target carries a stray point 1.3 km out at resolution 1.0 (the input of
    parity_checks.check_vgicp_edge_cases: 1291 cells per axis, more than INT_MAX in all) makes the whole call HGS_ERR_UNSUPPORTED, names the pair and
    the grid; the same call without that pair gives the reference records."""
    import parity_checks as PC
    tgt = synth.make_pair("VLP-16", 1, downsample=0.4)[0]
    wide, spans = PC.span_target(tgt, (1291, 1291, 1291), PC.vgicp_coord(1.0))
    assert list(spans) == [1291] * 3
    w = case.e.upload(wide)
    g = guesses(case.name)
    idx = [0, 1, 2, 3]
    tg = [case.dev[PAIRS[i][0]] for i in idx]
    sr = [case.dev[PAIRS[i][1]] for i in idx]
    gs = [g[i] for i in idx]
    rec, rc = case.e.align_pairs(tg[:2] + [w] + tg[2:], sr[:2] + [case.dev["c0"]] + sr[2:], gs[:2] + [g[0]] + gs[2:], MAX_RANGE, return_status=True)
    assert rc == L.HGS_ERR_UNSUPPORTED
    msg = L.lib().hgs_last_error(case.e._h).decode()
    assert "pair 2" in msg and "1291 x 1291 x 1291" in msg, msg
    assert_pairs_equal(case.e.align_pairs(tg, sr, gs, MAX_RANGE), reference(case.name), (case.name, "without the oversized pair"), idx=idx)
    w.close()


# ------------------------------------------------------------------------------------------------ LoopDetector.detect
def _run_detect(pnh, old, new, last_edge):
    ld = LoopDetector(pnh)
    calls = {"groups": 0, "pairs": 0, "batch": 0}
    reg = ld.registration

    def count(name, f):
        def g(*a, **kw):
            calls[name] += 1
            return f(*a, **kw)
        return g
    reg.loop_match_groups, reg.align_pairs, reg.loop_match_batch = count("groups", reg.loop_match_groups), count("pairs", reg.align_pairs), count("batch", reg.loop_match_batch)
    ld.last_edge_accum_distance = last_edge
    kfs = [KeyFrame(c, e, a, id=i) for i, (c, e, a) in enumerate(old)]
    nks = [KeyFrame(c, e, a, id=len(old) + i) for i, (c, e, a) in enumerate(new)]
    loops = ld.detect(kfs, nks)
    out = [(nks.index(l.key1), kfs.index(l.key2), l.relative_pose.tobytes()) for l in loops]
    result = (out, ld.last_edge_accum_distance, ld.last_detect_grouped, dict(calls))
    reg.close()
    return result


def check_detect(method):
    """Check 6: check_detect's scene under an engine the grouped call refuses, with reg_hip_batch_new_keyframes and reg_hip_batch_pairs: the loops,
    their order, their relative poses (bitwise) and the final last_edge_accum_distance equal the sequential detect; one refused grouped call, one
    pairs call, no loop_match_batch.  With the new key off, the refused grouped call is followed by today's loop."""
    pnh = {"registration_method": method, "reg_resolution": 1.0, "fitness_score_thresh": 2.5, "fitness_score_max_range": 4.0, "distance_thresh": 1.6,
           "accum_distance_thresh": 8.0, "min_edge_interval": 5.0}
    old, new = GC._detect_scene(8, [(-1.0, 103.0), (0.0, 110.0), (0.5, 112.0), (1.5, 120.0), (2.5, 126.0)], 1.0)
    seq = _run_detect(pnh, old, new, 100.0)
    both = _run_detect(dict(pnh, reg_hip_batch_new_keyframes=True, reg_hip_batch_pairs=True), old, new, 100.0)
    assert seq[0] == both[0] and seq[1] == both[1], (seq[0], both[0], seq[1], both[1])
    found = [l[0] for l in seq[0]]
    assert len(found) >= 2 and 0 not in found, found                   # (the first new keyframe fails the last-edge gate at entry)
    assert not seq[2] and seq[3] == {"groups": 0, "pairs": 0, "batch": len(found)}
    assert both[2] and both[3] == {"groups": 1, "pairs": 1, "batch": 0}, both[3]
    alone = _run_detect(dict(pnh, reg_hip_batch_pairs=True), old, new, 100.0)          # the new key acts only together with the other
    assert alone == seq, (alone[1:], seq[1:])
    off = _run_detect(dict(pnh, reg_hip_batch_new_keyframes=True), old, new, 100.0)
    assert off[:3] == seq[:3] and off[3] == {"groups": 1, "pairs": 0, "batch": len(found)}, off[3]


# ------------------------------------------------------------------------------------------------ LockstepOdometry
def check_lockstep_odometry(name):
    """Check 7: three streams over different scenes, six sweeps each, VLP-16 at ~1 m voxels; the streams move at different speeds, so they switch
    keyframes at different sweeps; every stream's poses are bitwise those of a ScanMatchingOdometry on its own engine.  NDT_OMP runs at resolution
    3.0 here: sweeps voxelised at 1 m hold ~1 600 points, too few for a single valid NDT cell at resolution 1.0 (the registration would end at its
    guess without an iteration and no stream would ever switch)."""
    make_params = _params(L.HGS_NDT_OMP, 3.0, L.HGS_DIRECT7) if name.startswith("NDT") else METHODS[name]
    speeds = (0.12, 0.22, 0.4)                                          # metres per sweep; keyframe_delta_trans 0.5: switches at sweeps 5 | 3 | 2 and 4
    kw = dict(keyframe_delta_trans=0.5, keyframe_delta_angle=10.0, keyframe_delta_time=100.0)
    sweeps = []
    for s, v in enumerate(speeds):
        sc = synth.make_scene(21 + s)
        sweeps.append([synth.voxel_downsample(synth.scan(sc, "VLP-16", synth.pose_matrix([v * k, 0.02 * k, 0.0], [0.0, 0.0, 0.004 * k * (s + 1)]), 300 + 10 * s + k), 1.0)
                       for k in range(6)])
    single, switches = [], []
    for s in range(len(speeds)):
        e = RegistrationHIP(make_params())
        od = ScanMatchingOdometry(e, **kw)
        poses, n_kf = [], []
        for k in range(6):
            poses.append(od.matching(0.1 * k, e.upload(sweeps[s][k])).tobytes())
            n_kf.append(od.num_keyframes)
        single.append(poses)
        switches.append([k for k in range(1, 6) if n_kf[k] != n_kf[k - 1]])
        e.close()
    assert all(switches) and len({tuple(w) for w in switches}) == len(speeds), switches     # every stream switches, no two at the same sweeps
    e = RegistrationHIP(make_params())
    calls = []
    pairs = e.align_pairs
    e.align_pairs = lambda *a, **k: (calls.append(len(a[0])), pairs(*a, **k))[1]
    lock = LockstepOdometry(e, len(speeds), **kw)
    for k in range(6):
        odoms = lock.matching(0.1 * k, [e.upload(sweeps[s][k]) for s in range(len(speeds))])
        for s in range(len(speeds)):
            assert odoms[s].tobytes() == single[s][k], (name, s, k)
    assert calls == [3] * 5 and [st.num_keyframes for st in lock.streams] == [1 + len(w) for w in switches]
    e.close()


# ------------------------------------------------------------------------------------------------ the C++ caller
def write_cpp_inputs(name, tmp_path):
    """The scene's clouds, the pair list and the guesses as files for tests/cpp/align_pairs_main.cpp; returns its arguments from guesses.bin on."""
    s = GC.scene()
    ids = {k: i for i, k in enumerate(s.clouds)}
    args = []
    for k, c in s.clouds.items():
        c.tofile(tmp_path / f"{k}.bin")
        args.append(f"C:{tmp_path / (k + '.bin')}")
    np.stack([L.colmajor16(g) for g in guesses(name)]).astype(np.float32).tofile(tmp_path / "guesses.bin")
    args += [f"P:{ids[t]}:{ids[src]}" for t, src in PAIRS]
    return [str(tmp_path / "guesses.bin"), *args]


def cpp_arguments(name, tmp_path):
    """<method> <neighbor_search> <resolution> <max_range> <guesses.bin> C:... P:... for one of METHODS"""
    p = METHODS[name]()
    return [str(p.method), str(p.neighbor_search), repr(float(p.resolution)), repr(MAX_RANGE), *write_cpp_inputs(name, tmp_path)]


CPP_METHODS = ["FAST_GICP", "NDT_OMP_DIRECT7", "FAST_VGICP_DIRECT7"]


def check_cpp_output(lines, name):
    """align_pairs_main prints every record as hex words, with the fitness pass (F) and without (N): equal to check 1's."""
    ref = reference(name)
    full = np.frombuffer(bytes.fromhex("".join(l.split()[2] for l in lines if l.startswith("F "))), dtype=L.RESULT_DTYPE)
    assert_pairs_equal(full, ref, (name, "C++ with fitness"))
    plain = np.frombuffer(bytes.fromhex("".join(l.split()[2] for l in lines if l.startswith("N "))), dtype=L.RESULT_DTYPE)
    assert_pairs_equal(plain, ref, (name, "C++ without fitness"), with_fitness=False)
