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
