"""ICP_HIP (HGS_ICP) on the MI355X against the restatement of tests/icp_reference.py: the vlp16 / hdl32 / hdl32_raw pairs of
tests/test_hip_parity.py with reciprocal correspondences off and on, the stage hook, a 64-candidate loop-closure batch against the
sequential reference with the same selection, the pcl::Registration adapter through tests/cpp/icp_adapter_main.cpp, and the shared checks of
tests/icp_checks.py on the solve step (hgs_debug_icp_step), the exact threshold rule, awkward sources, degenerate scenes and the fitness behind an
align — the same ones tests/test_icp_simt_host.py runs on the host emulation."""
import os
import subprocess

import numpy as np
import pytest

import icp_checks as IC
import icp_reference as IR
import oracle as O
from hdl_graph_slam_amd import synth, workloads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(kind):
    from test_hip_parity import _pair as parity_pair
    return parity_pair(kind)


def _engine(p):
    from hdl_graph_slam_amd.registration import RegistrationHIP
    return RegistrationHIP(p)


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("kind", ["vlp16", "hdl32", "hdl32_raw"])
def test_icp_align_equals_the_reference(kind, reciprocal):
    tgt, src, T = _pair(kind)
    p = IC.icp_params(reciprocal)
    e = _engine(p)
    e.setInputTarget(tgt)
    e.setInputSource(src)
    ref = IC.reference(p, tgt, src)
    for g in (np.eye(4), T @ synth.pose_matrix([0.3, -0.2, 0.05], [0.01, -0.005, 0.03])):
        IC.check_align(e, ref, g)
    again = e.align(np.eye(4))
    first = e.align(np.eye(4))
    assert bytes(again.final_transformation) == bytes(first.final_transformation)     # fixed reduction order
    e.close()


@pytest.mark.parametrize("reciprocal", [False, True])
def test_icp_correspondence_hook_equals_the_reference(reciprocal):
    tgt, src, T = _pair("hdl32")
    p = IC.icp_params(reciprocal)
    e = _engine(p)
    e.setInputTarget(tgt)
    e.setInputSource(src)
    ref = IC.reference(p, tgt, src)
    for pose in (np.eye(4), T):
        IC.check_correspond(e, ref, pose)
    e.close()


def test_icp_batch_of_64_candidates_against_the_sequential_reference():
    wl = workloads.make_loop_closure_set("HDL-32E", 0, n_candidates=64, downsample=0.25)
    p = IC.icp_params()
    e = _engine(p)
    e.setInputTarget(wl.target)
    cands = [e.upload(c) for c in wl.candidates]
    max_range = 1.0
    rec, best = e.loop_match_batch(cands, wl.guesses, max_range)
    fit = O.OracleRegistration(O.default_params(O.HGS_FAST_GICP))
    fit.setInputTarget(wl.target)
    scores = np.full(64, IR.DBL_MAX)
    conv = np.zeros(64, bool)
    for i, c in enumerate(wl.candidates):
        o = IC.reference(p, wl.target, c).align(wl.guesses[i])
        assert (int(rec[i]["iterations"]), bool(rec[i]["converged"])) == (o["iterations"], o["converged"]), i
        dt, dr = synth.pose_error(rec[i]["final_transformation"].reshape(4, 4).T.astype(np.float64), o["T"].astype(np.float32).astype(np.float64))
        assert dt <= IC.POSE_TOL and dr <= IC.POSE_TOL, (i, dt, dr)
        fit.setInputSource(c)
        scores[i] = fit.getFitnessScore(max_range, T=o["T"].astype(np.float32))
        conv[i] = o["converged"]
        assert abs(rec[i]["fitness_score"] - scores[i]) <= 1e-6 * scores[i], (i, rec[i]["fitness_score"], scores[i])
    want, bs = -1, IR.DBL_MAX
    for i in range(64):                     # loop_detector.hpp:146-153: skip non-converged, skip score > best, ties replace
        if conv[i] and scores[i] <= bs:
            bs, want = scores[i], i
    assert best == want or abs(scores[best] - scores[want]) <= 1e-6 * scores[want], (best, want, scores[best], scores[want])
    # bitwise independent of the batch: the first six again as a batch of six, and one by one
    IC.check_batch(e, cands[:6], wl.candidates[:6], wl.guesses[:6], p, wl.target, max_range)
    rec6, _ = e.loop_match_batch(cands[:6], wl.guesses[:6], max_range)
    assert rec6.tobytes() == rec[:6].tobytes()
    for c in cands:
        c.close()
    e.close()


@pytest.mark.parametrize("reciprocal", [0, 1])
def test_icp_adapter_matches_python_mirror(tmp_path, reciprocal):
    from hdl_graph_slam_amd import build as hip_build
    from hdl_graph_slam_amd.registrations import select_registration_method
    lib = hip_build.build_lib()
    exe = os.path.join(ROOT, "tests", "cpp", "icp_adapter_main")
    src_cpp = os.path.join(ROOT, "tests", "cpp", "icp_adapter_main.cpp")
    deps = [src_cpp, os.path.join(ROOT, "adapters", "registration_hip.hpp"), os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "tests", "mock_pcl"), "-I", os.path.join(ROOT, "tests", "mock_eigen"), "-I",
                        os.path.join(ROOT, "include"), src_cpp, "-o", exe, "-L", os.path.dirname(lib), "-lhgs_hip", f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    tgt, src, T = synth.make_pair("VLP-16", 1, downsample=0.3)
    tgt.tofile(tmp_path / "t.bin")
    src.tofile(tmp_path / "s.bin")
    out = subprocess.run([exe, str(reciprocal), str(tmp_path / "t.bin"), str(tmp_path / "s.bin")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "name hgs_hip::ICP"
    f = out[1].split()
    assert f[0] == "params" and (int(f[1]), int(f[2]), float(f[3]), float(f[4]), float(f[5]), int(f[6])) == (3, 64, 0.01, 0.0, 2.5, reciprocal)
    reg = select_registration_method({"registration_method": "ICP_HIP", "reg_use_reciprocal_correspondences": bool(reciprocal)})
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    r = reg.align(np.eye(4))
    c = out[2].split()
    assert (int(c[1]), int(c[3]), int(c[5])) == (r.converged, r.iterations, r.lm_tries)
    Tc = np.array([float(v) for v in out[3].split()], np.float32).reshape(4, 4).T
    assert np.array_equal(Tc, r.matrix())
    reg.close()


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
    tgt, src, T = synth.make_pair("VLP-16", 1, downsample=0.45)
    IC.check_fitness_after_align(_make, tgt, src, T @ synth.pose_matrix([0.3, -0.2, 0.05], [0.01, -0.005, 0.03]), reciprocal)
