"""ICP_HIP (HGS_ICP) on the CPU: the product kernels k_icp_correspond / k_icp_solve and the engine's ICP branch, compiled for the host against
the SIMT emulation of tests/emul and driven through the C-ABI and the Python mirror, against the restatement of tests/icp_reference.py on
pairs of at most ~6.5 k points: the align with reciprocal correspondences off and on, identity and non-identity guesses; the stage hook;
the < 3 correspondences and max_iterations exits; a 6-candidate loop-closure batch against six single aligns; and the shared checks of
tests/icp_checks.py on the solve step (hgs_debug_icp_step: every branch of svd3, the decision table of icp_after_pass), the exact
max_correspondence_distance rule, small / non-finite / empty / duplicated sources, degenerate scenes and the fitness behind an align."""
import numpy as np
import pytest

import icp_checks as IC
from hdl_graph_slam_amd import synth

simt = pytest.importorskip("emul.simt", reason="needs tests/emul")


@pytest.fixture(scope="module", autouse=True)
def simt_library():
    """Points the package's loader at tests/emul/libhgs_simt.so for the duration of this module (and back afterwards)."""
    path = simt.build()
    if path is None:
        pytest.skip("clang++ not available: the emulation build needs ext_vector_type / elementwise builtins")
    from hdl_graph_slam_amd import _lib as L
    saved = (L.LIB_PATH, L._lib)
    L.LIB_PATH, L._lib = path, None
    yield path
    L.LIB_PATH, L._lib = saved


def _engine(p):
    from hdl_graph_slam_amd.registration import RegistrationHIP
    return RegistrationHIP(p)


def _pair(kind):
    if kind == "vlp16":
        return synth.make_pair("VLP-16", 1, downsample=0.45)     # ~3.6 k points
    return synth.make_pair("HDL-32E", 4, downsample=0.5)         # ~6 k points


def _guesses(T):
    return [np.eye(4), T @ synth.pose_matrix([0.3, -0.2, 0.05], [0.01, -0.005, 0.03])]


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("kind", ["vlp16", "hdl32"])
def test_icp_align_equals_the_reference(kind, reciprocal):
    tgt, src, T = _pair(kind)
    for eps in (0.01, 1e-7):                 # the factory default, and a tight one that runs the iterations out to the MSE test
        p = IC.icp_params(reciprocal, transformation_epsilon=eps)
        e = _engine(p)
        e.setInputTarget(tgt)
        e.setInputSource(src)
        ref = IC.reference(p, tgt, src)
        for g in _guesses(T):
            IC.check_align(e, ref, g)
        e.close()


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_correspondence_hook_equals_the_reference(reciprocal):
    tgt, src, T = _pair("hdl32")
    p = IC.icp_params(reciprocal)
    e = _engine(p)
    e.setInputTarget(tgt)
    e.setInputSource(src)
    ref = IC.reference(p, tgt, src)
    for pose in (np.eye(4), T, T @ synth.pose_matrix([0.5, 0.2, -0.1], [0.02, 0.01, -0.05])):
        sums, corr = IC.check_correspond(e, ref, pose)
        assert sums[0] > 100
    e.close()


def test_icp_fewer_than_three_pairs_does_not_converge():
    tgt, src, T = _pair("vlp16")
    p = IC.icp_params(max_correspondence_distance=0.05)
    e = _engine(p)
    e.setInputTarget(tgt)
    e.setInputSource(src)
    far = synth.pose_matrix([40.0, 0.0, 0.0], [0.0, 0.0, 0.0])     # everything out of range: no pair at all
    r, o = IC.check_align(e, IC.reference(p, tgt, src), far)
    assert (r.converged, r.iterations, r.lm_tries) == (0, 0, 1)
    assert np.array_equal(r.matrix(), far.astype(np.float32))       # the pose is kept
    e.close()


def test_icp_max_iterations_counts_as_converged():
    tgt, src, T = _pair("vlp16")
    p = IC.icp_params(max_iterations=2, transformation_epsilon=1e-12)
    e = _engine(p)
    e.setInputTarget(tgt)
    e.setInputSource(src)
    r, o = IC.check_align(e, IC.reference(p, tgt, src), np.eye(4))
    assert (r.converged, r.iterations) == (1, 2)
    e.close()


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_loop_match_batch_equals_single_aligns(reciprocal):
    tgt, _, _ = _pair("vlp16")
    p = IC.icp_params(reciprocal)
    e = _engine(p)
    e.setInputTarget(tgt)
    srcs, guesses = [], []
    for k in range(6):
        _, s, T = synth.make_pair("VLP-16", 1 + k, downsample=0.45)
        srcs.append(s)
        guesses.append(T @ synth.pose_matrix([0.1 * k, -0.05 * k, 0.0], [0.0, 0.0, 0.01 * k]))
    cands = [e.upload(s) for s in srcs]
    IC.check_batch(e, cands, srcs, guesses, p, tgt, max_range=1.0)
    for c in cands:
        c.close()
    e.close()


# ---- the solve step through hgs_debug_icp_step, the threshold rule, small / awkward sources, degenerate geometry, fitness behind an align
def _make(p, src=None, tgt=None):
    e = _engine(p)
    if tgt is not None:
        e.setInputTarget(tgt)
    if src is not None:
        e.setInputSource(src)
    return e


def test_icp_step_hook_needs_a_source_and_the_icp_method():
    IC.check_step_hook_errors(_make)


@pytest.fixture(scope="module")
def step_engine():
    e = _make(IC.icp_params(), IC.hook_source())
    yield e
    e.close()


@pytest.mark.parametrize("case", IC.UMEYAMA_CASES)
def test_icp_umeyama_step_on_synthesised_sums(step_engine, case):
    IC.check_umeyama_step(step_engine, case)


def test_icp_after_pass_decision_table():
    IC.check_decision_table(lambda p: _make(p, IC.hook_source()))


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_threshold_rule_is_exact(reciprocal):
    IC.check_threshold_rule(_make, reciprocal)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_small_sources(reciprocal):
    IC.check_small_sources(_make, reciprocal)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_non_finite_source_rows(reciprocal):
    IC.check_non_finite_rows(_make, reciprocal)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_empty_source(reciprocal):
    IC.check_empty_source(_make, reciprocal)


def test_icp_duplicated_points_under_the_reciprocal_test():
    IC.check_duplicated_points(_make)


def test_icp_degenerate_geometry():
    IC.check_degenerate_geometry(_make)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_fitness_behind_an_align_equals_the_oracle(reciprocal):
    tgt, src, T = _pair("vlp16")
    IC.check_fitness_after_align(_make, tgt, src, T @ synth.pose_matrix([0.3, -0.2, 0.05], [0.01, -0.005, 0.03]), reciprocal)
