"""Shared checks of hgs_detect_floor_batch (the k_flb_* kernels of hgs_kernels.hip, detect_floor_batch_impl of hgs_engine.hip, the Python mirror
FloorDetector.detect_batch, LockstepOdometry with a floor detector and tests/cpp/floor_batch_main.cpp).  tests/test_floor_batch_gpu.py runs them on the
MI355X, tests/test_floor_batch_simt_host.py on the host emulation of the same kernels.  `make(pnh, **constants)` builds a hdl_graph_slam_amd.FloorDetector
on the library under test.

Two yardsticks, every cloud of every batch against both, none skipped:
  * the single call: hgs_detect_floor of that cloud alone on a FRESH engine — the record as bytes (ransac_iterations included), the filtered and the
    inlier cloud through download().  Bits, no tolerance.
  * the restatement of tests/floor_reference.py per cloud, under floor_checks.compare's rules.

The mixed batch (clouds(), about 12 k points; generator np.random.default_rng(11), drawn in this order, constructions of floor_checks.patch_cloud and
floor_checks.check_rejections): patch_cloud() (3000 points, 30 % floor); flat patches z = -2 +- 1 cm over +-10 m of 700, 300, 255, 256, 257, 513, 2 and 9
points; a wall of 2000 points at x ~ 5; clutter(1500, 200): 200 floor points among 1300 clutter points; an empty cloud.  floor_reference.detect on them
(check_reference_is_not_trivial asserts the properties, not these numbers): without the normal filter all four reasons appear — DETECTED (patch3000 after
168 hypotheses, 700 and 513 after 1), NOT_VERTICAL (the wall, 2), TOO_FEW_INLIERS (the clutter, all 1000), TOO_FEW_POINTS (everything below 512 points,
0); with it and floor_pts_thresh 3 the filter removes points (434 of 3000 at 94 hypotheses, 295 of 1500 at 604), the wall and the 2-point cloud are left
with nothing, the 9-point cloud runs with k = 9 < normal_k, and 255 / 256 / 257 points sit on the tile edge of the count kernel and the compactions.

The 2-point patch under the normal filter: pcl::NormalEstimation gives a point with fewer than three neighbours a NaN normal, which fails the filter, so the
filter keeps nothing of a clipped cloud of fewer than three points (floor_normals_defined, hgs_floor.h) — n_filtered 0, as the reference has it."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

import floor_checks as FC
import floor_reference as FR
from hdl_graph_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_SETS = {"no_normals": {"use_normal_filtering": False}, "normals_thresh3": {"floor_pts_thresh": 3}}
FLAT_SIZES = (700, 300, 255, 256, 257, 513, 2, 9)
FIELDS = ["x", "y", "z", "intensity"]


# ---- inputs (computed once, read-only)
@functools.lru_cache(maxsize=None)
def clouds() -> dict:
    rng = np.random.default_rng(11)
    out = {"patch3000": FC.patch_cloud()}
    for n in FLAT_SIZES:
        out[f"flat{n}"] = FC.records(np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), -2.0 + rng.uniform(-0.01, 0.01, n)], 1))
    out["wall"] = FC.records(np.stack([np.full(2000, 5.0) + rng.uniform(-0.01, 0.01, 2000), rng.uniform(-5, 5, 2000), rng.uniform(-2.9, -1.1, 2000)], 1))
    n, nf = 1500, 200
    floor = np.stack([rng.uniform(-10, 10, nf), rng.uniform(-10, 10, nf), -2.0 + rng.uniform(-0.02, 0.02, nf)], 1)
    clutter = np.stack([rng.uniform(-10, 10, n - nf), rng.uniform(-10, 10, n - nf), rng.uniform(0.15, 0.99, n - nf) * rng.choice([-1.0, 1.0], n - nf) - 2.0], 1)
    out["clutter"] = FC.records(np.concatenate([floor, clutter])[rng.permutation(n)])
    out["empty"] = np.zeros(0, synth.POINT_XYZI_DTYPE)
    for c in out.values():
        c.setflags(write=False)
    return out


MIXED = ("patch3000",) + tuple(f"flat{n}" for n in FLAT_SIZES) + ("wall", "clutter", "empty")


def _key(pnh, constants):
    return tuple(sorted(pnh.items())), tuple(sorted(constants.items()))


@functools.lru_cache(maxsize=None)
def _reference_cached(name, key) -> FR.Floor:
    return FR.detect(FC.ref_params(dict(key[0]), **dict(key[1])), clouds()[name])


def reference(name, pnh, **constants) -> FR.Floor:
    """tests/floor_reference.py on one cloud of the set (computed once per parameter set, needs no device)."""
    return _reference_cached(name, _key(pnh, constants))


class Outcome:
    """What one cloud gave: the record's bytes, the downloaded filtered cloud and the inlier cloud (None: no floor)."""

    def __init__(self, record, filtered, inliers):
        self.last, self.record = record, bytes(record)
        self.filtered, self.inliers = filtered, inliers

    def filtered_points(self):
        return self.filtered

    def floor_points(self):
        return self.inliers

    def coeffs(self):
        return np.array(self.last.coeffs, dtype=np.float32) if self.last.detected else None


_SINGLE = {}


def single(make, name, pnh, **constants) -> Outcome:
    """The first yardstick: hgs_detect_floor of the cloud alone on a fresh engine (computed once per library under test, read-only)."""
    key = (make.__module__, name, _key(pnh, constants))
    if key not in _SINGLE:
        d = make(pnh, **constants)
        d.detect(clouds()[name])
        _SINGLE[key] = Outcome(d.last, d.filtered_points(), d.floor_points())
        d.close()
    return _SINGLE[key]


def outcomes(d, n) -> list:
    return [Outcome(d.last_batch[i], d.filtered_points(i), d.floor_points(i)) for i in range(n)]


def same_cloud(a, b, label):
    assert (a is None) == (b is None), label
    if a is not None:
        assert len(a) == len(b) and a[FIELDS].tobytes() == b[FIELDS].tobytes(), label


def assert_equals_yardsticks(make, got: Outcome, name, pnh, label="", **constants):
    want = single(make, name, pnh, **constants)
    assert got.record == want.record, (label, name, "record", [getattr(got.last, f) for f, _ in got.last._fields_][1:], [getattr(want.last, f) for f, _ in want.last._fields_][1:])
    same_cloud(got.filtered, want.filtered, (label, name, "filtered cloud"))
    same_cloud(got.inliers, want.inliers, (label, name, "inlier cloud"))
    FC.compare(got, got.coeffs(), reference(name, pnh, **constants), clouds()[name])


def run_batch(make, d, names, pnh, label="", **constants) -> list:
    """One detect_batch of the named clouds (host arrays, uploaded for the call) on detector d; every cloud against both yardsticks — all of them are
    looked at before the first mismatch is raised, so that a report names every cloud that differs."""
    co = d.detect_batch([clouds()[n] for n in names])
    got = outcomes(d, len(names))
    assert len(co) == len(names)
    failures = []
    for k, name in enumerate(names):
        try:
            assert_equals_yardsticks(make, got[k], name, pnh, label, **constants)
        except AssertionError as exc:
            failures.append((k, name, str(exc).splitlines()[0] if str(exc) else repr(exc)))
        assert (co[k] is None) == (got[k].coeffs() is None) and (co[k] is None or co[k].tobytes() == got[k].coeffs().tobytes())
    assert not failures, (label, failures)
    return got


# ---- 0. the reference alone
def check_reference_is_not_trivial():
    a = {n: reference(n, PARAM_SETS["no_normals"]) for n in MIXED}
    b = {n: reference(n, PARAM_SETS["normals_thresh3"]) for n in MIXED}
    assert {r.reason for r in a.values()} == {FR.DETECTED, FR.TOO_FEW_POINTS, FR.TOO_FEW_INLIERS, FR.NOT_VERTICAL}
    assert len({r.ransac_iterations for r in a.values()}) >= 4
    assert 0 in {r.ransac_iterations for r in a.values()} and 1000 in {r.ransac_iterations for r in a.values()}     # stops at once / runs to max_iterations, side by side
    assert any(r.n_filtered < r.n_clipped for r in b.values()) and any(0 < r.n_filtered < r.n_clipped for r in b.values())
    assert b["flat9"].detected and b["flat9"].n_clipped == 9 and b["wall"].n_filtered == 0 and b["flat2"].reason == FR.TOO_FEW_POINTS
    assert all(b[f"flat{n}"].detected for n in (255, 256, 257))
    for r in list(a.values()) + list(b.values()):
        assert r.ransac is None or not r.ransac.near


# ---- 1. the batch equals the single calls
def check_batch_equals_single_calls(make, params, reverse):
    pnh = PARAM_SETS[params]
    names = MIXED[::-1] if reverse else MIXED
    d = make(pnh)
    got = run_batch(make, d, names, pnh)
    assert len(got[names.index("empty")].filtered) == 0 and got[names.index("empty")].last.reason == FR.TOO_FEW_POINTS
    assert d.batch_stats()["clouds"] == len(names)
    d.close()


# ---- 2. chunking and grouping, small iteration limits
def check_chunking_and_grouping(make):
    pnh = PARAM_SETS["no_normals"]
    d = make(pnh)
    blobs = []
    for chunk, group in ((64, 0), (1, 0), (7, 0), (1000, 0), (64, 1), (64, 3)):
        d.engine.set_option("floor_chunk", chunk)
        d.engine.set_option("floor_batch_group", group)
        got = run_batch(make, d, MIXED, pnh, (chunk, group))
        blobs.append(b"".join(g.record for g in got))
        st = d.batch_stats()
        n_ransac = st["ransac_clouds"]
        groups = 1 if group == 0 else -(-n_ransac // group)
        assert st["readbacks"] == 2 + (groups - 1), (chunk, group, st)         # clip, final; one more per further group
    assert len(set(blobs)) == 1
    d.close()
    for max_it in (0, 1, 5):
        dm = make(pnh, ransac_max_iterations=max_it)
        for chunk, group in ((64, 0), (1, 3)):
            dm.engine.set_option("floor_chunk", chunk)
            dm.engine.set_option("floor_batch_group", group)
            got = run_batch(make, dm, MIXED, pnh, (max_it, chunk, group), ransac_max_iterations=max_it)
            assert max(g.last.ransac_iterations for g in got) == max_it
        dm.close()


# ---- 3. repeats, one cloud, no cloud, calls back to back, the handle's state
def check_repeats_and_back_to_back(make):
    pnh = PARAM_SETS["no_normals"]
    d = make(pnh)
    e = d.engine
    dc = e.upload(clouds()["patch3000"])
    d.detect_batch([dc, dc, dc])                              # the same DeviceCloud three times
    for g in outcomes(d, 3):
        assert_equals_yardsticks(make, g, "patch3000", pnh, "one cloud three times")
    run_batch(make, d, ("flat700",), pnh, "one cloud")
    assert d.detect_batch([]) == [] and d.last_batch == [] and d.batch_stats() == dict(clouds=0, ransac_clouds=0, ransac_rounds=0, readbacks=0)
    # the handle's target and source, a single call and a prefilter around three batches of different shapes
    tgt, src = e.upload(FC.scan("vlp16")), e.upload(synth.make_pair("VLP-16", 1, downsample=0.3)[1])
    e.setInputTarget(tgt)
    e.setInputSource(src)
    align_before = bytes(e.align(np.eye(4, dtype=np.float32)))
    raw = synth.make_pair("VLP-16", 2)[0][::8].copy()
    pre_before = e.prefilter(raw)
    run_batch(make, d, MIXED, pnh, "first batch")
    d.detect(dc)
    assert bytes(d.last) == single(make, "patch3000", pnh).record
    same_cloud(d.floor_points(), single(make, "patch3000", pnh).inliers, "the single call between two batches")
    run_batch(make, d, ("clutter", "flat9", "wall"), pnh, "second batch")
    run_batch(make, d, ("flat513", "empty", "flat513", "patch3000", "flat2"), pnh, "third batch")
    assert bytes(e.align(np.eye(4, dtype=np.float32))) == align_before
    pre_after = e.prefilter(raw)
    same_cloud(pre_after.download(), pre_before.download(), "prefilter() behind the batches")
    d.detect(dc)
    assert bytes(d.last) == single(make, "patch3000", pnh).record
    for c in (dc, tgt, src, pre_before, pre_after):
        c.close()
    d.close()


# ---- 4. structure: read-backs do not grow with the number of clouds
def check_structure(make):
    for params in PARAM_SETS:
        pnh = PARAM_SETS[params]
        d = make(pnh)
        stats = {}
        for n in (2, 9):
            run_batch(make, d, ("flat700",) * n, pnh, f"{n} x flat700")
            stats[n] = d.batch_stats()
            assert (stats[n]["clouds"], stats[n]["ransac_clouds"]) == (n, n)
        assert stats[2]["readbacks"] == stats[9]["readbacks"] == (3 if pnh.get("use_normal_filtering", True) else 2), stats
        assert stats[2]["ransac_rounds"] > 0 and stats[9]["ransac_rounds"] > 0
        run_batch(make, d, MIXED, pnh, "mixed")
        assert d.batch_stats()["ransac_clouds"] == sum(reference(n, pnh).reason != FR.TOO_FEW_POINTS for n in MIXED)
        d.close()


# ---- 5. the batched prefilter's resident output goes in
def check_resident_input(make):
    d = make({})
    raws = [synth.make_pair("VLP-16", s)[0] for s in (2, 3, 4)]
    dcs = d.engine.prefilter_batch(raws)
    co = d.detect_batch(dcs)
    n_detected = 0
    for i, dc in enumerate(dcs):
        cloud = dc.download()
        ref = FR.detect(FC.ref_params({}), cloud)
        assert ref.n_clipped > 500
        got = Outcome(d.last_batch[i], d.filtered_points(i), d.floor_points(i))
        FC.compare(got, co[i], ref, cloud)
        n_detected += int(ref.detected)
    assert n_detected >= 2
    for dc in dcs:
        dc.close()
    d.close()


# ---- 6. refusals touch nothing
def raw_batch(d, handles, n=None, null_clouds=False, null_out=False, params=None, engine=None):
    """hgs_detect_floor_batch itself.  Returns (status, the two cloud arrays as integers — prefilled with a sentinel, the records' bytes — prefilled with 0xAB)."""
    from hdl_graph_slam_amd import _lib as L
    count = len(handles) if n is None else n
    size = max(count, len(handles), 1)
    arr = (C.c_void_p * size)(*handles)
    res = (L.HgsFloorResult * size)()
    C.memset(res, 0xAB, C.sizeof(res))
    f, i = (C.c_void_p * size)(*([0xdead] * size)), (C.c_void_p * size)(*([0xdead] * size))
    rc = L.lib().hgs_detect_floor_batch((engine or d.engine)._h, None if null_clouds else arr, count, C.byref(params if params is not None else d.params),
                                        None if null_out else res, f, i)
    return rc, [v or 0 for v in f] + [v or 0 for v in i], bytes(res)


def check_refusals(make):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.floor_detection import floor_params_from_rosparams
    pnh = PARAM_SETS["no_normals"]
    d, other = make(pnh), make(pnh)
    good = d.engine.upload(clouds()["flat700"])
    tiny = d.engine.upload(clouds()["flat2"])
    foreign = other.engine.upload(clouds()["flat700"])
    gone = make(pnh)
    orphan = gone.engine.upload(clouds()["flat9"])
    gone.close()                                              # hgs_destroy orphans the cloud; the handle stays valid until it is destroyed
    refused = {
        "a NULL cloud array": dict(handles=[good._h.value, good._h.value], null_clouds=True),
        "a NULL record array": dict(handles=[good._h.value, good._h.value], null_out=True),
        "a NULL entry": dict(handles=[good._h.value, None, good._h.value]),
        "a cloud of another handle": dict(handles=[good._h.value, foreign._h.value]),
        "an orphaned cloud": dict(handles=[orphan._h.value, good._h.value]),
        "invalid parameters": dict(handles=[good._h.value], params=floor_params_from_rosparams(pnh, normal_k=2)),
        "a negative threshold": dict(handles=[good._h.value], params=floor_params_from_rosparams({"floor_pts_thresh": -1})),
        "more clouds than HGS_FLOOR_BATCH_MAX_CLOUDS": dict(handles=[tiny._h.value] * 4097),
    }
    # (more than 2^30 points in total: not produced — it would need resident clouds of 16 GB)
    for what, kw in refused.items():
        rc, arrays, recs = raw_batch(d, **kw)
        assert rc == L.HGS_ERR_INVALID_ARGUMENT, (what, rc)
        assert all(v == 0 for v in arrays[:len(kw["handles"])]) and all(v == 0 for v in arrays[len(arrays) // 2:][:len(kw["handles"])]), (what, "a cloud array entry is not NULL")
        assert recs == b"\xab" * len(recs), (what, "a record was written")
        run_batch(make, d, ("flat700", "empty", "patch3000"), pnh, "after the refusal of " + what)            # the engine stays usable
    rc, arrays, _ = raw_batch(d, [tiny._h.value] * 4096)       # the limit itself
    assert rc == L.HGS_OK and all(arrays[:4096]) and not any(arrays[4096:])
    for v in arrays[:4096]:
        L.lib().hgs_cloud_destroy(v)
    assert raw_batch(d, [], null_clouds=True, null_out=True)[0] == L.HGS_OK                                    # n_clouds == 0
    assert foreign.size == 700 and other.detect(foreign) is not None                                           # the other engine's cloud was left alone
    for c in (good, tiny, foreign, orphan):
        c.close()
    d.close()
    other.close()


# ---- 7. the Python mirror, LockstepOdometry with a floor detector
def check_python_mirror(make):
    pnh = PARAM_SETS["normals_thresh3"]
    d = make(pnh)
    names = ("patch3000", "flat9", "wall", "clutter")
    resident = d.engine.upload(clouds()["flat9"])
    co = d.detect_batch([clouds()["patch3000"], resident, clouds()["wall"], clouds()["clutter"]])       # host arrays and a DeviceCloud mixed
    assert resident.size == 9                                  # the caller's cloud is not closed
    recs = [bytes(r) for r in d.last_batch]
    fps, ips = [d.filtered_points(i) for i in range(4)], [d.floor_points(i) for i in range(4)]
    for k, name in enumerate(names):
        one = d.detect(clouds()[name])                         # (detect drops the batch's clouds: they were downloaded above)
        assert (one is None) == (co[k] is None) and (one is None or (one.dtype == np.float32 and one.tobytes() == co[k].tobytes()))
        assert bytes(d.last) == recs[k]
        same_cloud(d.filtered_points(), fps[k], name)
        same_cloud(d.floor_points(), ips[k], name)
    assert co[2] is None and co[0] is not None and co[0].shape == (4,)
    resident.close()
    d.close()


def check_lockstep_odometry(make):
    """Two streams of raw sweeps (every 4th ray of a VLP-16): LockstepOdometry with prefilter_params and a floor detector on its engine runs one detect_batch
    per sweep time; last_floors are those of detect per stream on the same filtered sweeps, the odoms those of a run without the detector."""
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.odometry import LockstepOdometry
    from hdl_graph_slam_amd.registration import RegistrationHIP
    import prefilter_checks as PFC
    pnh = {"floor_pts_thresh": 100}
    p = PFC.device_params(downsample_resolution=0.5, outlier_removal_method=0)
    kw = dict(keyframe_delta_trans=0.5, keyframe_delta_angle=10.0, keyframe_delta_time=100.0)
    raw = [[synth.scan(synth.make_scene(21 + s), "VLP-16", synth.pose_matrix([v * k, 0.02 * k, 0.0], [0.0, 0.0, 0.004 * k * (s + 1)]), 300 + 10 * s + k)[::4].copy()
            for k in range(3)] for s, v in enumerate((0.12, 0.3))]

    def run(with_detector):
        from hdl_graph_slam_amd import FloorDetector
        e = RegistrationHIP(L.default_params(L.HGS_FAST_GICP))
        d = FloorDetector(pnh, engine=e) if with_detector else None       # on the odometry's engine: the prefiltered sweeps go in resident
        seen, calls = [], []
        batch = e.prefilter_batch
        e.prefilter_batch = lambda c, *a, **k: (lambda out: (seen.append([o.download() for o in out]), out)[1])(batch(c, *a, **k))
        if d is not None:
            detect_batch = d.detect_batch
            d.detect_batch = lambda c: (calls.append(len(c)), detect_batch(c))[1]
        lock = LockstepOdometry(e, 2, prefilter_params=p, floor_detector=d, **kw)
        odoms, floors = [], []
        for k in range(3):
            sw = [raw[0][k], raw[1][k] if k != 1 else None]    # a stream without a sweep at one time
            odoms.append([None if o is None else o.tobytes() for o in lock.matching(0.1 * k, sw)])
            floors.append(list(lock.last_floors))
        if d is not None:
            d.close()
        e.close()
        return odoms, floors, seen, calls

    odoms0, floors0, _, _ = run(False)
    odoms1, floors1, seen, calls = run(True)
    assert odoms0 == odoms1 and all(f == [None, None] for f in floors0)
    assert calls == [2, 1, 2]
    one = make(pnh)
    n_floor = 0
    for k in range(3):
        have = [0, 1] if k != 1 else [0]
        assert k != 1 or floors1[k][1] is None
        for j, s in enumerate(have):
            want = one.detect(seen[k][j])
            got = floors1[k][s]
            assert (want is None) == (got is None) and (want is None or want.tobytes() == got.tobytes()), (k, s)
            n_floor += want is not None
    assert n_floor >= 3
    one.close()


# ---- 8. the C++ caller
def fnv1a(records) -> int:
    h = 1469598103934665603
    if records is None:
        return h
    data = np.stack([np.ascontiguousarray(records[f]).view(np.uint32) for f in FIELDS], axis=1).tobytes() if len(records) else b""
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def check_cpp_caller(make, tmp_path, lib, exe_name, link_name):
    """tests/cpp/floor_batch_main.cpp: hgs_detect_floor_batch through the C header alone; its records, counts and checksums are those of the mirror's single
    calls, and it finds its own single calls (a second engine) identical."""
    exe = os.path.join(ROOT, "tests", "cpp", exe_name)
    src = os.path.join(ROOT, "tests", "cpp", "floor_batch_main.cpp")
    deps = [src, os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(dep) > os.path.getmtime(exe) for dep in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-l" + link_name,
                        f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    for params in PARAM_SETS:
        pnh = PARAM_SETS[params]
        args = [str(int(pnh.get("use_normal_filtering", True))), str(pnh.get("floor_pts_thresh", 512))]
        for name in MIXED:
            clouds()[name].tofile(tmp_path / f"{name}.bin")
            args.append(str(tmp_path / f"{name}.bin"))
        out = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(MIXED) + 1, out
        n_ransac = 0
        for i, name in enumerate(MIXED):
            w = single(make, name, pnh)
            r = w.last
            co = np.array(r.coeffs, dtype=np.float32).view(np.uint32)
            want = [str(i), str(r.detected), str(r.reason), str(r.n_clipped), str(r.n_filtered), str(r.n_inliers), str(r.ransac_iterations)]
            want += [f"{int(v):08x}" for v in co]
            want += [str(len(w.filtered)), f"{fnv1a(w.filtered):016x}", str(-1 if w.inliers is None else len(w.inliers)), f"{fnv1a(w.inliers):016x}", "identical", "1"]
            assert out[i].split() == want, (params, name, out[i], want)
            n_ransac += r.reason != FR.TOO_FEW_POINTS
        stats = out[-1].split()
        assert stats[:3] == ["stats", str(len(MIXED)), str(n_ransac)] and int(stats[4]) == (3 if pnh.get("use_normal_filtering", True) else 2), out[-1]
