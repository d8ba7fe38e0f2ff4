"""Shared ICP parity assertions: the device engine (HGS_ICP on an MI355X, or the same kernels emulated on the host by tests/emul)
against the test-side restatement of tests/icp_reference.py on identical inputs."""
from __future__ import annotations

import numpy as np

import icp_reference as IR
from hdl_graph_slam_amd import _lib as L, synth

POSE_TOL = 1e-6


def icp_params(reciprocal=False, **kw):
    p = L.default_params(L.HGS_ICP)
    p.use_reciprocal_correspondences = reciprocal
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def reference(p, tgt, src) -> IR.IcpReference:
    ref = IR.IcpReference.from_params(p)
    ref.setInputTarget(tgt)
    ref.setInputSource(src)
    return ref


def check_align(engine, ref, guess, tol=POSE_TOL):
    """Equal iterations, passes and convergence flag; pose within tol m / rad of the reference (the device hands it over in float);
    the result's error is the last iteration's mse."""
    r = engine.align(guess)
    o = ref.align(guess)
    assert (r.iterations, bool(r.converged), r.lm_tries) == (o["iterations"], o["converged"], o["passes"]), \
        ((r.iterations, r.converged, r.lm_tries), (o["iterations"], o["converged"], o["passes"]))
    dt, dr = synth.pose_error(r.matrix().astype(np.float64), o["T"].astype(np.float32).astype(np.float64))
    assert dt <= tol and dr <= tol, (dt, dr)
    if o["iterations"] > 0:
        assert abs(r.error - o["mse"]) <= 1e-9 * max(1.0, o["mse"]), (r.error, o["mse"])
    else:
        assert r.error == IR.DBL_MAX
    return r, o


def _d2(a, b) -> np.ndarray:
    return ((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(axis=1)


def check_correspond(engine, ref, T, max_mismatch=0.002):
    """hgs_debug_icp_correspond against the reference pass: equal correspondence indices, except where the test shows a float-ulp tie or a
    distance on the max_correspondence_distance threshold; the 17 sums equal the sums over the device's own pairs, and the Umeyama step from
    them equals the step from the pairs."""
    T = np.asarray(T, np.float64)
    sums, corr = engine.icp_correspond(T)
    want = ref.correspondences(T)
    bad = np.nonzero(corr != want)[0]
    assert len(bad) <= max(2, max_mismatch * len(want)), f"{len(bad)} / {len(want)} correspondences differ"
    moved = IR.move(T, ref.src)
    pos = {int(i): k for k, i in enumerate(ref.src_idx)}
    rel = 1e-5
    for i in bad:
        p = moved[pos[int(i)]][None]
        a, b = int(corr[i]), int(want[i])
        if a >= 0 and b >= 0:                       # two targets at the same distance
            da, db = _d2(p, ref.tgt[[a]])[0], _d2(p, ref.tgt[[b]])[0]
            assert abs(da - db) <= rel * max(da, db, 1e-12), (i, a, b, da, db)
            continue
        j = a if a >= 0 else b
        dj = _d2(p, ref.tgt[[j]])[0]
        on_threshold = abs(dj - ref.max_corr2) <= rel * ref.max_corr2
        nearer = ref._t.nn_target(p)[1][0]         # the pair's target is not the nearest one: a forward tie
        forward_tie = abs(dj - float(nearer)) <= rel * max(dj, 1e-12) and b < 0 and a >= 0 and not ref.reciprocal
        reverse_tie = False
        if ref.reciprocal:
            r = IR.unmove(T, ref.tgt[[j]])
            back_d2 = float(ref._s.nn_target(r)[1][0])
            self_d2 = _d2(r, ref.src[[pos[int(i)]]])[0]
            reverse_tie = abs(self_d2 - back_d2) <= rel * max(self_d2, 1e-12) or abs(self_d2 - ref.max_corr2) <= rel * ref.max_corr2
        assert on_threshold or forward_tie or reverse_tie, (i, a, b, dj)
    # the sums over the device's own pairs
    keep = corr[ref.src_idx] >= 0
    p = moved[keep]
    q = ref.tgt[corr[ref.src_idx][keep]]
    want_sums = IR.IcpReference.sums(p, q, _d2(p, q))
    assert sums[0] == want_sums[0]
    np.testing.assert_allclose(sums[1:16], want_sums[1:16], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(sums[16], want_sums[16], rtol=1e-6)
    if sums[0] >= 3:
        np.testing.assert_allclose(IR.umeyama_from_sums(sums), IR.umeyama(p, q), atol=1e-8)
    return sums, corr


def check_batch(engine, candidates, src_clouds, guesses, params, tgt, max_range=None):
    """hgs_loop_match_batch: every record bitwise equal to a single align of that candidate followed by hgs_fitness, and the sequential rule's
    best index; the poses also against the reference."""
    max_range = L.DBL_MAX if max_range is None else max_range
    rec, best = engine.loop_match_batch(candidates, guesses, max_range)
    fields = ("final_transformation", "converged", "iterations", "error", "lm_tries")
    scores = []
    for i, src in enumerate(src_clouds):
        engine.setInputSource(candidates[i])
        r = engine.align(guesses[i])
        for f in fields:
            a = np.asarray(rec[i][f])
            b = np.asarray(getattr(r, f)) if f != "final_transformation" else np.array(r.final_transformation, np.float32)
            assert a.tobytes() == np.asarray(b, a.dtype).tobytes(), (i, f, a, b)
        s = engine.getFitnessScore(max_range)
        assert rec[i]["fitness_score"] == s, (i, rec[i]["fitness_score"], s)
        scores.append(s)
        o = reference(params, tgt, src).align(guesses[i])
        assert (int(rec[i]["iterations"]), bool(rec[i]["converged"])) == (o["iterations"], o["converged"])
    want = -1
    bs = L.DBL_MAX
    for i in range(len(scores)):
        if not rec[i]["converged"] or scores[i] > bs:
            continue
        bs, want = scores[i], i
    assert best == want, (best, want)
    return rec, best


# ------------------------------------------------------------------------------------------------ the solve step on synthesised sums
def sums_of(p, q, d2_sum=0.0) -> np.ndarray:
    """The 17 sums of a pass whose pairs are (p_i, q_i), in double (the points need not be floats here)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    return np.concatenate([[len(p)], p.sum(0), q.sum(0), (q.T @ p).reshape(9), [d2_sum]])


def _rot(rpy) -> np.ndarray:
    return synth.pose_matrix([0.0, 0.0, 0.0], rpy)[:3, :3]


def _moved(p, R, t):
    return p @ R.T + t


def umeyama_case(name):
    """(p, q, R, t, kind) of one input of the Umeyama step.  kind: "numpy" — centred, rank >= 2: the step is unique and the numpy restatement
    states it to ~1e-15; "far" — Sigma cancels, both are held to the known motion; "zero" — Sigma = 0 exactly; "rank1" — collinear points,
    the rotation is not unique."""
    rng = np.random.default_rng(17)
    R, t = _rot([0.1, -0.2, 0.7]), np.array([1.0, -2.0, 0.5])
    if name == "full_rank":
        p = rng.normal(0, 5, (200, 3))
        return p, _moved(p, R, t), R, t, "numpy"
    if name == "identity":
        p = rng.normal(0, 5, (200, 3))
        return p, p.copy(), np.eye(3), np.zeros(3), "numpy"
    if name == "coplanar_z0":                      # z = 0 exactly on both sides: Sigma's last row and column are exactly 0
        p = np.c_[rng.normal(0, 5, (200, 2)), np.zeros(200)]
        Rz, tz = _rot([0.0, 0.0, 0.4]), np.array([0.7, -0.3, 0.0])
        q = _moved(p, Rz, tz)
        q[:, 2] = 0.0
        return p, q, Rz, tz, "numpy"
    if name == "coplanar_tilted":
        p = np.c_[rng.normal(0, 5, (200, 2)), np.zeros(200)] @ _rot([0.5, -0.3, 0.2]).T
        return p, _moved(p, R, t), R, t, "numpy"
    if name == "three_points":
        p = np.array([[1.0, 0.2, -0.3], [-2.0, 1.5, 0.4], [0.5, -1.0, 2.0]])
        return p, _moved(p, R, t), R, t, "numpy"
    if name == "mirror":                           # q is a mirror image of p (thin third axis): Eigen's rule flips the smallest direction
        p = rng.normal(0, 1, (200, 3)) * [5.0, 3.0, 0.2]
        return p, p @ (np.diag([1.0, 1.0, -1.0]) @ R).T, None, None, "numpy"
    if name == "equal_singular_values":            # the 8 corners of a cube
        p = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
        return p, p @ R.T, R, np.zeros(3), "numpy"
    if name == "small_scale":
        p = rng.normal(0, 5e-4, (200, 3))
        return p, _moved(p, R, t * 1e-4), R, t * 1e-4, "numpy"
    if name == "far_from_origin":                  # a milliradian motion seen from (1000, 2000, -50)
        p = rng.normal(0, 5, (200, 3)) + [1000.0, 2000.0, -50.0]
        Rm, tm = _rot([1e-3, -2e-3, 1.5e-3]), np.array([0.02, -0.01, 0.005])
        return p, _moved(p, Rm, tm), Rm, tm, "far"
    if name == "zero_matrix":                      # 256 equal points with short mantissas: every sum and mean is exact, Sigma = 0 exactly
        p, q = np.tile([1.5, -2.25, 0.5], (256, 1)), np.tile([3.0, 0.75, -1.25], (256, 1))
        return p, q, np.eye(3), q[0] - p[0], "zero"
    if name == "rank1":
        u = np.array([1.0, 2.0, -2.0]) / 3.0
        p = np.outer(rng.uniform(-5, 5, 200), u) + [0.3, -0.2, 0.1]
        return p, _moved(p, R, t), R, t, "rank1"
    if name == "rank1_axis":                       # a vertical pole: two rows and two columns of Sigma are (nearly) 0
        p = np.c_[np.full(200, 2.0), np.full(200, 3.0), rng.uniform(0, 5, 200)]
        return p, p + [0.25, -0.125, 0.5], np.eye(3), np.array([0.25, -0.125, 0.5]), "rank1"
    raise KeyError(name)


UMEYAMA_CASES = ("full_rank", "identity", "coplanar_z0", "coplanar_tilted", "three_points", "mirror", "equal_singular_values", "small_scale",
                 "far_from_origin", "zero_matrix", "rank1", "rank1_axis")


def check_umeyama_step(engine, name):
    """hgs_debug_icp_step (the product kernel k_icp_solve) from the identity on the sums of one case: Delta is a finite proper rotation + t;
    unique steps equal tests/icp_reference.umeyama_from_sums within 1e-12 (a double-precision host build of hgs_icp.h measured <= 1.2e-15; the
    margin is for another correct rounding of sqrt and division on the device).  Returns (|dR|max, |dt|max) against the numpy restatement, or for
    "far" the device's and numpy's errors against the known motion."""
    p, q, R_true, t_true, kind = umeyama_case(name)
    sums = sums_of(p, q, float(((q - p) ** 2).sum()))
    T, converged, done, iterations, mse = engine.icp_step(sums, np.eye(4), IR.DBL_MAX, 0)
    assert np.isfinite(T).all() and np.isfinite(mse), (name, T, mse)
    assert iterations == 1, (name, iterations)
    np.testing.assert_array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
    R, t = T[:3, :3], T[:3, 3]
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12, (name, R @ R.T)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, (name, np.linalg.det(R))
    assert mse == sums[16] / sums[0], (name, mse)
    want = IR.umeyama_from_sums(sums)
    dR, dt = float(np.abs(R - want[:3, :3]).max()), float(np.abs(t - want[:3, 3]).max())
    if kind == "numpy":
        print(f"icp_step {name}: device - numpy |dR| {dR:.3g} |dt| {dt:.3g}")
        assert dR <= 1e-12 and dt <= 1e-12, (name, dR, dt)
        if R_true is not None:                     # (the restatement itself recovers the motion the points were made with)
            assert np.abs(want[:3, :3] - R_true).max() <= 1e-12 and np.abs(want[:3, 3] - t_true).max() <= 1e-11, name
        return dR, dt
    if kind == "far":
        dev = (float(np.abs(R - R_true).max()), float(np.abs(t - t_true).max()))
        ref = (float(np.abs(want[:3, :3] - R_true).max()), float(np.abs(want[:3, 3] - t_true).max()))
        print(f"icp_step {name}: against the known motion, device |dR| {dev[0]:.3g} |dt| {dev[1]:.3g}; numpy |dR| {ref[0]:.3g} |dt| {ref[1]:.3g}")
        assert dev[0] <= 4 * ref[0] + 1e-12 and dev[1] <= 4 * ref[1] + 1e-12, f"{name}: device (dR, dt) {dev}, numpy restatement {ref}"
        return dev, ref
    if kind == "zero":
        n = sums[0]
        assert not (sums[7:16].reshape(3, 3) / n - np.outer(sums[4:7] / n, sums[1:4] / n)).any(), "the case is built so that Sigma is exactly 0"
        np.testing.assert_array_equal(R, np.eye(3))
        np.testing.assert_array_equal(t, t_true)
        return 0.0, 0.0
    # rank 1: R takes the direction of p onto that of q, and every pair is met
    up, uq = p[-1] - p[0], q[-1] - q[0]
    up, uq = up / np.linalg.norm(up), uq / np.linalg.norm(uq)
    ddir = float(np.linalg.norm(R @ up - uq))
    res = float(np.linalg.norm(p @ R.T + t - q, axis=1).max())
    print(f"icp_step {name}: |R u_p - u_q| {ddir:.3g}, max residual {res:.3g}")
    assert ddir <= 1e-12 and res <= 1e-9, (name, ddir, res)
    return ddir, res


# ------------------------------------------------------------------------------------------------ the decision table of icp_after_pass
T_NONTRIVIAL = synth.pose_matrix([1.25, -0.5, 0.75], [0.03, -0.02, 0.4])


def _decision_sums(angle, trans, mse=0.25, n=50):
    """Sums whose Umeyama step is a rotation by `angle` about a fixed axis plus a translation of length `trans`, and whose mse is `mse`
    (n = 50 and mse = 0.25: sums[16] / sums[0] is exact)."""
    rng = np.random.default_rng(5)
    p = rng.normal(0, 3, (n, 3))
    p -= p.mean(0)
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    t = trans * np.array([0.6, 0.0, -0.8])
    return sums_of(p, p @ R.T + t, mse * n)


def check_step_against_reference(engine, params, sums, T_in, mse_prev, iterations_in):
    """One hgs_debug_icp_step against IcpReference.after_pass on the same state: flags, iteration count, mse, and the pose within 1e-12."""
    ref = IR.IcpReference.from_params(params)
    want = ref.after_pass(sums, T_in, mse_prev, iterations_in)
    T, converged, done, iterations, mse = engine.icp_step(sums, T_in, mse_prev, iterations_in)
    got = (bool(converged), bool(done), iterations)
    assert got == (want["converged"], want["done"], want["iterations"]), (got, want)
    if want["mse"] is None:
        assert T[:3].tobytes() == np.ascontiguousarray(np.asarray(T_in, np.float64)[:3]).tobytes(), "fewer than 3 pairs: the pose is kept bitwise"
    else:
        assert mse == want["mse"], (mse, want["mse"])
        np.testing.assert_allclose(T, want["T"], rtol=0, atol=1e-12 * max(1.0, np.abs(want["T"]).max()))
    return got


def check_decision_table(make_engine):
    """icp_after_pass through hgs_debug_icp_step.  make_engine(params) -> an engine with some source set.  Every expectation below is stated
    from PCL's DefaultConvergenceCriteria (tests/icp_reference.py) and checked against IcpReference.after_pass as well."""
    def run(e, p, sums, T_in=T_NONTRIVIAL, mse_prev=IR.DBL_MAX, it=0):
        return check_step_against_reference(e, p, sums, T_in, mse_prev, it)

    p = icp_params()                                # transformation_epsilon 0.01 -> rot_thr 0.99; rotation_epsilon 0
    e = make_engine(p)
    # translation: the SQUARED translation against the unsquared epsilon — 0.09^2 = 0.0081 <= 0.01 < 0.11^2 = 0.0121
    assert run(e, p, _decision_sums(0.0, 0.09)) == (True, True, 1)
    assert run(e, p, _decision_sums(0.0, 0.11)) == (False, False, 1)
    # rotation: cos 0.14 = 0.99022 >= 0.99 > cos 0.15 = 0.98877
    assert run(e, p, _decision_sums(0.14, 0.0)) == (True, True, 1)
    assert run(e, p, _decision_sums(0.15, 0.0)) == (False, False, 1)
    assert run(e, p, _decision_sums(0.14, 0.11)) == (False, False, 1)       # both tests have to hold
    # the absolute-MSE test, with a Delta too large for the transformation test: |mse - mse_prev| < 1e-12
    big = _decision_sums(0.3, 0.5, mse=0.25)
    for d, conv in ((5e-13, True), (-5e-13, True), (2e-12, False), (-2e-12, False)):
        assert run(e, p, big, mse_prev=0.25 + d, it=3) == (conv, conv, 4), d
    assert run(e, p, big, mse_prev=IR.DBL_MAX, it=3) == (False, False, 4)
    # max_iterations counts as converged whatever the Delta; one iteration earlier it does not
    assert run(e, p, big, it=p.max_iterations - 1) == (True, True, p.max_iterations)
    assert run(e, p, big, it=p.max_iterations - 2) == (False, False, p.max_iterations - 1)
    # fewer than 3 pairs: not converged, done, iterations unchanged, the pose bitwise kept (check_step_against_reference); exactly 3: a step
    two = sums_of([[1.0, 2.0, 3.0], [-1.0, 0.5, 2.0]], [[1.1, 2.0, 3.0], [-0.9, 0.5, 2.0]], 0.02)
    assert run(e, p, two, it=5) == (False, True, 5)
    assert run(e, p, np.zeros(17), it=5) == (False, True, 5)
    p3 = np.array([[1.0, 0.2, -0.3], [-2.0, 1.5, 0.4], [0.5, -1.0, 2.0]])
    assert run(e, p, sums_of(p3, p3 + [0.5, 0.0, 0.0], 0.75), it=5) == (False, False, 6)
    e.close()
    p = icp_params(rotation_epsilon=0.9999)         # cos 0.01 = 0.99995 >= 0.9999 > cos 0.02 = 0.9998
    e = make_engine(p)
    assert run(e, p, _decision_sums(0.01, 0.0)) == (True, True, 1)
    assert run(e, p, _decision_sums(0.02, 0.0)) == (False, False, 1)
    e.close()


# ------------------------------------------------------------------------------------------------ d2 <= max_corr^2, exact
def check_threshold_rule(make_engine, reciprocal):
    """PCL keeps a pair at d2 == max_corr^2 (2.5 m: 6.25 is exact in float) and drops it one float further; nothing is excused here.  With
    reciprocal correspondences the reverse search meets the same two distances.  Once against a target of one leaf, and once against a tree
    in which the point on the threshold is the near corner of a leaf's box (the walk's box test meets 6.25 as well)."""
    nf = np.nextafter(np.float32(2.5), np.float32(3.0))
    few = np.array([[2.5, 0, 0], [0, nf, 0], [20, 20, 0], [-20, 20, 5], [30, -10, 2], [-15, -25, 1], [12, 18, -3]], np.float32)
    rng = np.random.default_rng(41)
    ang, rad = rng.uniform(0, 2 * np.pi, 64), rng.uniform(15, 40, 64)
    behind = [[2.5 + 0.01 * k, 0.001 * k, 0] for k in range(1, 8)]                     # seven points behind target 0, seen from the origin
    tree = np.concatenate([few, np.array(behind, np.float32), np.c_[rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-3, 3, 64)].astype(np.float32)])
    # the origin: target 0 at exactly 2.5 m;  (0, 2 nf, 0): target 1 at nf (2 nf - nf is exact);  (0.5, nf, 0): target 1 at 0.5 m, and target 1's
    # nearest source point, so that no reverse search ends on the second point
    src = np.array([[0, 0, 0], [0, 2 * nf, 0], [0.5, nf, 0]], np.float32)
    assert np.float32(2.5) * np.float32(2.5) == np.float32(6.25) and np.float32(nf) * np.float32(nf) > np.float32(6.25)
    p = icp_params(reciprocal)
    assert p.max_correspondence_distance == 2.5
    for tgt in (few, tree):
        e = make_engine(p, src, tgt)
        sums, corr = e.icp_correspond(np.eye(4))
        assert list(corr) == [0, -1, 1], corr
        assert sums[0] == 2 and sums[16] == 6.25 + 0.25, sums
        np.testing.assert_array_equal(corr, reference(p, tgt, src).correspondences(np.eye(4)))
        # the same distances alone: a single pair on the threshold is kept, a single pair one float beyond it is not
        for s, want in ((src[:1], 0), (src[1:2], -1)):
            e.setInputSource(np.ascontiguousarray(s))
            sums, corr = e.icp_correspond(np.eye(4))
            assert list(corr) == [want] and sums[0] == (want >= 0), (corr, sums)
        e.close()


# ------------------------------------------------------------------------------------------------ small and awkward sources
SMALL_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 513)


def small_pair():
    tgt, src, T = synth.make_pair("VLP-16", 1, downsample=0.6)      # ~2 k points
    return synth.xyz_of(tgt).astype(np.float32), synth.xyz_of(src).astype(np.float32), T


def check_small_sources(make_engine, reciprocal):
    tgt, src, T = small_pair()
    assert len(src) >= max(SMALL_N)
    p = icp_params(reciprocal)
    e = make_engine(p, None, tgt)
    for n in SMALL_N:
        s = np.ascontiguousarray(src[:n])
        e.setInputSource(s)
        ref = reference(p, tgt, s)
        for pose in (np.eye(4), T):
            check_correspond(e, ref, pose)
        r, o = check_align(e, ref, T)
        if n < 3:
            assert (r.converged, r.iterations, r.lm_tries) == (0, 0, 1), n
            assert np.array_equal(r.matrix(), T.astype(np.float32)), n
    e.close()


def check_non_finite_rows(make_engine, reciprocal):
    tgt, src, T = small_pair()
    s = np.ascontiguousarray(src[:300]).copy()
    bad = [0, 63, 64, 299]
    s[0] = [np.nan, 1.0, 1.0]
    s[63] = [1.0, np.inf, 1.0]
    s[64] = [1.0, 1.0, -np.inf]
    s[299] = [np.nan, np.nan, np.nan]
    p = icp_params(reciprocal)
    e = make_engine(p, s, tgt)
    ref = reference(p, tgt, s)
    assert len(ref.src_idx) == 296
    for pose in (np.eye(4), T):
        sums, corr = check_correspond(e, ref, pose)
        assert (corr[bad] == -1).all(), corr[bad]
    check_align(e, ref, T)
    e.close()


def check_empty_source(make_engine, reciprocal):
    tgt, _, T = small_pair()
    s = np.zeros((0, 3), np.float32)
    p = icp_params(reciprocal)
    e = make_engine(p, s, tgt)
    r, o = check_align(e, reference(p, tgt, s), T)
    assert (o["converged"], o["iterations"], o["passes"]) == (False, 0, 1)
    assert np.array_equal(r.matrix(), T.astype(np.float32))
    e.close()


def check_duplicated_points(make_engine):
    """Every source and target point twice, reciprocal correspondences on: of two equal points the lowest index is the neighbour (the
    oracle's rule, tests/parity_checks.check_nn1_with_equidistant_targets), so the second copy of a source point never passes the
    reciprocal test.  Exact equality of the indices."""
    tgt, src, T = small_pair()
    t2 = np.ascontiguousarray(np.concatenate([tgt[:400], tgt[:400]]))
    s2 = np.ascontiguousarray(np.concatenate([src[:200], src[:200]]))
    p = icp_params(True)
    e = make_engine(p, s2, t2)
    ref = reference(p, t2, s2)
    for pose in (np.eye(4), T):
        sums, corr = e.icp_correspond(pose)
        want = ref.correspondences(pose)
        np.testing.assert_array_equal(corr, want)
        assert (corr[200:] == -1).all() and (corr[:200] < 400).all()
        assert sums[0] == (want >= 0).sum()
    assert (want >= 0).sum() >= 3
    e.close()


# ------------------------------------------------------------------------------------------------ degenerate geometry, both kernels
def _to_f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def floor_pair():
    rng = np.random.default_rng(23)
    g = np.stack(np.meshgrid(np.arange(40) * 0.5 - 10, np.arange(40) * 0.5 - 10), -1).reshape(-1, 2) + rng.uniform(-0.2, 0.2, (1600, 2))
    tgt = _to_f32(np.c_[g, np.zeros(len(g))])
    M = synth.pose_matrix([0.15, -0.1, 0.0], [0.0, 0.0, 0.02])
    src = tgt[::2].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    src[:, 2] = 0.0
    return tgt, _to_f32(src)


def mirror_pair():
    """A thin slab and its mirror image in z, turned a little: every point's nearest neighbour is its own image, so the pass's Sigma has
    det U det V < 0."""
    rng = np.random.default_rng(29)
    g = np.stack(np.meshgrid(np.arange(30) - 14.5, np.arange(30) - 14.5), -1).reshape(-1, 2) + rng.uniform(-0.1, 0.1, (900, 2))
    tgt = _to_f32(np.c_[g, rng.uniform(0.05, 0.2, 900) * rng.choice([-1.0, 1.0], 900)])
    src = (tgt.astype(np.float64) * [1.0, 1.0, -1.0]) @ _rot([0.0, 0.0, 0.004]).T
    return tgt, _to_f32(src)


def pole_pair():
    z = np.arange(400) * 0.0125
    tgt = _to_f32(np.c_[np.full(400, 2.0), np.full(400, 3.0), z])
    src = _to_f32(np.c_[np.full(200, 2.125), np.full(200, 2.9375), z[::2] + 0.03125])
    return tgt, src


def check_degenerate_geometry(make_engine):
    for max_iterations in (1, None):
        kw = {} if max_iterations is None else {"max_iterations": max_iterations}
        p = icp_params(**kw)
        tgt, src = floor_pair()
        e = make_engine(p, src, tgt)
        r, o = check_align(e, reference(p, tgt, src), np.eye(4))
        assert o["iterations"] >= 1
        e.close()
        if max_iterations == 1:
            tgt, src = mirror_pair()
            e = make_engine(p, src, tgt)
            ref = reference(p, tgt, src)
            _, _, mp, mq, _ = ref.correspond(np.eye(4))
            S = (mq - mq.mean(0)).astype(np.float64).T @ (mp - mp.mean(0)).astype(np.float64)
            U, _, Vt = np.linalg.svd(S)
            assert np.linalg.det(U) * np.linalg.det(Vt) < 0, "the case is built to need the reflection rule"
            r, o = check_align(e, ref, np.eye(4))
            assert (o["iterations"], o["converged"]) == (1, True)
            e.close()
        # pole only: the rotation is not unique — the result is a rotation that lays the source's line onto the target's
        tgt, src = pole_pair()
        e = make_engine(p, src, tgt)
        for guess in (np.eye(4), synth.pose_matrix([0.0, 0.0, 0.0], [0.02, -0.01, 0.0])):
            r = e.align(guess)
            assert r.iterations >= 1
            T = r.matrix().astype(np.float64)
            assert np.isfinite(T).all()
            R, t = T[:3, :3], T[:3, 3]
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(R) - 1.0) <= 1e-5, R
            assert np.linalg.norm(R @ [0.0, 0.0, 1.0] - [0.0, 0.0, 1.0]) <= 1e-5, R
            moved = src.astype(np.float64) @ R.T + t
            off = float(np.abs(moved[:, :2] - [2.0, 3.0]).max())
            assert off <= 1e-5, off
            again = e.align(guess)
            assert bytes(again.final_transformation) == bytes(r.final_transformation)
        e.close()


# ------------------------------------------------------------------------------------------------ fitness behind an align
def check_fitness_after_align(make_engine, tgt, src, guess, reciprocal):
    """hgs_fitness right behind an ICP align starts its search from corr[] — full of -1 with reciprocal correspondences — and has to give
    the oracle's score at the device's final pose all the same."""
    import oracle as O
    p = icp_params(reciprocal)
    e = make_engine(p, src, tgt)
    fit = O.OracleRegistration(O.default_params(O.HGS_FAST_GICP))
    fit.setInputTarget(tgt)
    fit.setInputSource(src)
    r = e.align(guess)
    assert r.iterations >= 1
    if reciprocal:
        _, corr = e.icp_correspond(r.matrix().astype(np.float64))
        assert (corr < 0).sum() > 0.1 * len(corr)               # (the seeds the fitness pass starts from do have holes)
        r = e.align(guess)
    for max_range in (1.0, L.DBL_MAX):
        got = e.getFitnessScore(max_range)
        want = fit.getFitnessScore(max_range, T=r.matrix())
        assert abs(got - want) <= 1e-6 * want, (max_range, got, want)
        assert e.last_num_inliers == fit.last_num_inliers, (max_range, e.last_num_inliers, fit.last_num_inliers)
    e.close()


# ------------------------------------------------------------------------------------------------ the test files' common cases
def hook_source() -> np.ndarray:
    """Some source for hgs_debug_icp_step: 300 points, i.e. two tile rows, of which the hook fills the first and zeroes the second."""
    return np.random.default_rng(1).uniform(-5, 5, (300, 3)).astype(np.float32)


def check_step_hook_errors(make_engine):
    from hdl_graph_slam_amd.registration import HgsError
    import pytest
    e = make_engine(icp_params())
    with pytest.raises(HgsError, match=L.STATUS[L.HGS_ERR_NO_SOURCE]):
        e.icp_step(np.zeros(17))
    e.setInputSource(hook_source()[:1])             # a source is all it needs: no target
    assert e.icp_step(np.zeros(17))[1:4] == (0, 1, 0)
    e.close()
    e = make_engine(L.default_params(L.HGS_FAST_GICP), hook_source())
    with pytest.raises(HgsError, match=L.STATUS[L.HGS_ERR_UNSUPPORTED]):
        e.icp_step(np.zeros(17))
    e.close()
