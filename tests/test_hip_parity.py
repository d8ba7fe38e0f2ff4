"""MI355X parity tests: the HIP path, called through the C-ABI of include/hgs_registration.h, against the CPU oracle on
identical seeded inputs.  Tolerance (north_star): final pose within 1e-3 m / 1e-3 rad; nearest-neighbour / correspondence
indices bit-exact.  Run with `pytest -m gpu` on a GPU box."""
import numpy as np
import pytest

import oracle as O
import parity_checks as PC
from hdl_graph_slam_amd import synth

pytestmark = pytest.mark.gpu


def _hip(params):
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP
    p = L.HgsParams()
    for name, _ in L.HgsParams._fields_:
        setattr(p, name, getattr(params, name))
    return RegistrationHIP(p)


def _pair(kind):
    if kind == "vlp16":      # BASELINE config 1 sized (hdl prefilter 0.1 m)
        return synth.make_pair("VLP-16", 2, downsample=0.1)
    if kind == "hdl32":
        return synth.make_pair("HDL-32E", 4, downsample=0.25)
    if kind == "hdl32_raw":  # BASELINE config 2: ~60 k-point HDL-32E pair, no downsample
        return synth.make_pair("HDL-32E", 5)
    if kind == "dense":
        return synth.make_dense_pair(3, 20000, extent=25.0)
    raise KeyError(kind)


@pytest.fixture(scope="module", params=["vlp16", "hdl32", "dense", "hdl32_raw"])
def gicp_case(request):
    tgt, src, T = _pair(request.param)
    p = O.default_params(O.HGS_FAST_GICP)
    e, o = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e, o, tgt, src)
    yield e, o, tgt, src, T
    e.close()


def test_tree_search_is_exact(gicp_case):
    e, o, tgt, src, T = gicp_case
    PC.check_nn(e, o, synth.xyz_of(src)[::3])
    PC.check_nn(e, o, np.array([[1e4, 0, 0], [0, -5e3, 30], [0, 0, 0], [1e-3, 1e-3, 1e-3]], np.float32))
    # every target point is its own nearest neighbour at distance 0 (duplicates resolve to the lower index)
    idx, d2 = e.nn_target(synth.xyz_of(tgt))
    assert np.all(d2 == 0) and np.all(idx <= np.arange(len(tgt)))


def test_covariances(gicp_case):
    e, o, tgt, src, T = gicp_case
    PC.check_covariances(e, tgt)


def test_covariances_with_equidistant_neighbours():
    """Regular grids and duplicated points: the k-th distance is shared by up to 8 points of which up to 7 belong to the k
    nearest; the set the covariance is summed over must be the oracle's (ties -> lowest original index)."""
    cloud = PC.tie_heavy_cloud()
    for k in (20, 10):
        p = O.default_params(O.HGS_FAST_GICP)
        p.correspondence_randomness = k
        e = _hip(p)
        e.setInputTarget(cloud)
        PC.check_covariances(e, cloud, k)
        e.close()


def test_covariances_with_both_gather_passes():
    PC.check_covariances_both_gathers(_hip)


@pytest.mark.gpu
def test_split_regularisation_kernel_equals_the_inline_one():
    PC.check_cov_split_equals_inline(_hip)


def test_covariances_of_short_last_packets_and_short_packet_launches():
    PC.check_covariances_with_short_packets(_hip)


@pytest.mark.gpu
def test_two_launch_lm_rounds_equal_the_four_launch_rounds():
    PC.check_two_launch_rounds_equal_four_launch_rounds(_hip, reps=20)


def test_covariances_when_the_leaf_log_overflows():
    """k_knn_cov with lanes whose k-NN ball covers hundreds of leaves: the gather pass falls back from the logged leaves to the tree."""
    PC.check_covariances_with_outliers(_hip)


@pytest.mark.parametrize("method", [O.HGS_REG_PLANE, O.HGS_REG_NORMALIZED_MIN_EIG, O.HGS_REG_NONE])
def test_covariance_regularization_methods(method):
    """fast_gicp::RegularizationMethod other than the FROBENIUS default: covariances, one linearisation and a full
    registration against the oracle; FAST_VGICP inherits the point covariances."""
    tgt, src, T = _pair("vlp16")
    p = O.default_params(O.HGS_FAST_GICP)
    p.regularization_method = method
    e, o = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e, o, tgt, src)
    PC.check_covariances(e, tgt, 20, method)
    if method != O.HGS_REG_NONE:   # raw covariances of coplanar neighbourhoods are singular: not a usable GICP metric
        # covariances with a 1e-3 : 1 spectrum stored as floats: the Mahalanobis sum carries their 6e-8 rounding amplified
        PC.check_gicp_linearize(e, o, T.astype(np.float32).astype(np.float64), err_rel=2e-5)
        PC.check_align(e, o, T @ synth.pose_matrix([0.2, -0.1, 0.02], [0.002, -0.003, 0.015]), tol_m=1e-5, tol_rad=1e-5)
    e.close()
    if method == O.HGS_REG_PLANE:
        pv = O.default_params(O.HGS_FAST_VGICP)
        pv.regularization_method = method
        e, o = _hip(pv), O.OracleRegistration(pv)
        PC.load_pair(e, o, tgt, src)
        PC.check_gicp_linearize(e, o, T.astype(np.float32).astype(np.float64), err_rel=2e-5)
        e.close()


def test_gicp_linearize(gicp_case):
    e, o, tgt, src, T = gicp_case
    PC.check_gicp_linearize(e, o, T.astype(np.float32).astype(np.float64))
    PC.check_gicp_linearize(e, o, np.eye(4))


@pytest.mark.parametrize("guess_kind", ["identity", "near"])
def test_gicp_align(gicp_case, guess_kind):
    e, o, tgt, src, T = gicp_case
    guess = np.eye(4) if guess_kind == "identity" else T @ synth.pose_matrix([0.2, -0.1, 0.02], [0.002, -0.003, 0.015])
    re, ro = PC.check_align(e, o, guess, tol_m=1e-5, tol_rad=1e-5)
    PC.check_fitness(e, o, ro.matrix())
    # align()'s output cloud = T * source
    out = e.transformed_source(re.matrix())
    ref = synth.xyz_of(src).astype(np.float64) @ re.matrix()[:3, :3].astype(np.float64).T + re.matrix()[:3, 3]
    assert np.abs(out[:, :3] - ref).max() < 1e-4


def test_gicp_lm_rejection_path(gicp_case):
    e, o, tgt, src, T = gicp_case
    p = O.default_params(O.HGS_FAST_GICP)
    p.max_correspondence_distance = 1.0
    p.transformation_epsilon, p.rotation_epsilon = 1e-5, 1e-6
    e2, o2 = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e2, o2, tgt, src)
    guess = T @ synth.pose_matrix([0.8, 0.5, 0.1], [0.01, 0.01, 0.08])
    PC.check_align(e2, o2, guess, tol_m=1e-4, tol_rad=1e-4)
    e2.close()


def test_gicp_run_to_run_determinism(gicp_case):
    e, o, tgt, src, T = gicp_case
    a = e.align(np.eye(4))
    b = e.align(np.eye(4))
    assert bytes(a.final_transformation) == bytes(b.final_transformation) and a.error == b.error


def test_gicp_point_order_invariance(gicp_case):
    """Property: registration does not depend on the order of the source points (sums are re-associated only)."""
    e, o, tgt, src, T = gicp_case
    ra = e.align(np.eye(4)).matrix()
    rng = np.random.default_rng(0)
    e.setInputSource(src[rng.permutation(len(src))])
    rb = e.align(np.eye(4)).matrix()
    e.setInputSource(src)
    dt, dr = synth.pose_error(ra, rb)
    assert dt < 1e-5 and dr < 1e-5


@pytest.fixture(scope="module", params=[("hdl32", 1.0, O.HGS_DIRECT1), ("vlp16", 0.5, O.HGS_DIRECT7), ("dense", 1.0, O.HGS_DIRECT27), ("hdl32_raw", 1.0, O.HGS_DIRECT1)])
def vgicp_case(request):
    kind, res, search = request.param
    tgt, src, T = _pair(kind)
    p = O.default_params(O.HGS_FAST_VGICP)
    p.resolution, p.neighbor_search = res, search
    e, o = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e, o, tgt, src)
    yield e, o, tgt, src, T
    e.close()


def test_vgicp_linearize(vgicp_case):
    """FastVGICP (registrations.cpp:48-56): voxel lookups bit-exact (count of voxel correspondences per source point),
    H / b / error to the accuracy of the float-stored covariances."""
    e, o, tgt, src, T = vgicp_case
    PC.check_gicp_linearize(e, o, T.astype(np.float32).astype(np.float64))
    PC.check_gicp_linearize(e, o, np.eye(4))


@pytest.mark.parametrize("guess_kind", ["identity", "near"])
def test_vgicp_align(vgicp_case, guess_kind):
    e, o, tgt, src, T = vgicp_case
    guess = np.eye(4) if guess_kind == "identity" else T @ synth.pose_matrix([0.2, -0.1, 0.02], [0.002, -0.003, 0.015])
    re, ro = PC.check_align(e, o, guess, tol_m=1e-5, tol_rad=1e-5)
    PC.check_fitness(e, o, ro.matrix())
    a = e.align(guess)
    assert bytes(a.final_transformation) == bytes(re.final_transformation)   # run-to-run determinism


@pytest.mark.parametrize("name", sorted(PC.vgicp_voxel_cases()))
def test_vgicp_voxel_map(name):
    """The target's Gaussian voxel map itself — coordinates, point counts, means, covariances of every voxel — against the float64 numpy reference
    (parity_checks.check_vgicp_voxels), on small targets built to hit the map build's edges (parity_checks.vgicp_voxel_cases)."""
    res, cloud, input_check = PC.vgicp_voxel_cases()[name]
    p = O.default_params(O.HGS_FAST_VGICP)
    p.resolution = res
    e = _hip(p)
    PC.check_vgicp_voxels(e, cloud, res, input_check)
    e.close()


def test_vgicp_edge_cases():
    """Empty / far / one-point / non-finite / tiny / sparse / boundary inputs, extreme resolutions, a mixed loop batch, a target swap and the size
    limit of the voxel grid (parity_checks.check_vgicp_edge_cases)."""
    PC.check_vgicp_edge_cases(_hip)


@pytest.fixture(scope="module", params=[("hdl32", 1.0, O.HGS_DIRECT7), ("hdl32", 0.5, O.HGS_DIRECT1), ("vlp16", 1.0, O.HGS_DIRECT7), ("hdl32_raw", 1.0, O.HGS_DIRECT7),
                                        ("hdl32", 1.0, O.HGS_KDTREE)])
def ndt_case(request):
    kind, res, search = request.param
    tgt, src, T = _pair(kind)
    p = O.default_params(O.HGS_NDT_OMP)
    p.resolution, p.neighbor_search = res, search
    e, o = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e, o, tgt, src)
    yield e, o, tgt, src, T, kind, p
    e.close()


def test_ndt_cells(ndt_case):
    e, o, *_ = ndt_case
    PC.check_ndt_cells(e, o)


def test_ndt_derivatives(ndt_case):
    e, o, tgt, src, T, kind, p = ndt_case
    for p6 in ([T[0, 3], T[1, 3], T[2, 3], 0.003, -0.004, 0.02], [T[0, 3] + 0.1, T[1, 3], T[2, 3], 3.14, 3.13, 3.1], [0, 0, 0, 0, 0, 0]):
        PC.check_ndt_derivatives(e, o, np.array(p6, np.float64), rel=1e-10)


def test_ndt_align(ndt_case):
    """End-to-end NDT parity, every run to convergence: twelve guesses per case (identity, ground truth, ten perturbations),
    bit-identical to the oracle's exact-sum mode and within 1e-3 m / 1e-3 rad of its serial-sum (ndt_omp) mode — see
    parity_checks.check_ndt_to_convergence.  What makes this possible: per-point terms are bit-faithful (float operation
    order, fixed-sequence exp, libm-independent Euler angles), and the sum over the points is an exact integer accumulation
    whose result does not depend on tiling or on the order the atomics land in."""
    e, o, tgt, src, T, kind, p = ndt_case
    report = []
    rows = PC.check_ndt_to_convergence(e, p, tgt, src, PC.ndt_guesses(T, 12, seed=3), bitwise=p.neighbor_search != O.HGS_KDTREE, report=report,
                                       label=f"{kind} res {p.resolution} search {p.neighbor_search}")
    assert max(r["iterations"] for r in rows) >= 13   # long runs are part of the comparison
    PC.write_report(f"ndt_parity_{kind}_{p.resolution}_{p.neighbor_search}.json", report)
    PC.check_fitness(e, o, T.astype(np.float32))
    a, b = e.align(np.eye(4)), e.align(np.eye(4))
    assert bytes(a.final_transformation) == bytes(b.final_transformation)   # run-to-run determinism (atomics are integer adds)


@pytest.mark.parametrize("kind", ["vlp16", "hdl32"])
def test_ndt_line_search_follows_the_oracle(kind):
    """hgs_params.ndt_line_search = 1 (a working More-Thuente search, opt-in): same iterations, derivative passes and pose as
    the oracle's loop."""
    tgt, src, T = _pair(kind)
    p = O.default_params(O.HGS_NDT_OMP)
    p.resolution, p.ndt_line_search = 1.0, 1
    e, o = _hip(p), O.OracleRegistration(p)
    PC.load_pair(e, o, tgt, src)
    for off in ([0.0, 0.0, 0.0, 0.0], [0.3, 0.1, 0.0, 0.02], [0.1, -0.05, 0.0, 0.01], [0.02, 0.01, 0.0, 0.002]):
        re, ro = PC.check_align(e, o, T @ synth.pose_matrix(off[:3], [0, 0, off[3]]), tol_m=1e-6, tol_rad=1e-6)
        assert ro.lm_tries >= ro.iterations + 1
    e.close()


def test_edge_cases():
    p = O.default_params(O.HGS_FAST_GICP)
    e = _hip(p)
    from hdl_graph_slam_amd.registration import HgsError
    with pytest.raises(HgsError):
        e.align(np.eye(4))                       # no target / source yet
    tgt = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 1], [np.inf, 1, 1]], np.float32)
    e.setInputTarget(tgt)
    idx, d2 = e.nn_target(np.array([[0.9, 0.1, 0.0], [0.1, 0.1, 0.8]], np.float32))
    assert list(idx) == [1, 4]
    e.setInputSource(np.zeros((0, 3), np.float32))  # empty source: terminates, reports non-convergence or zero motion
    r = e.align(np.eye(4))
    assert r.iterations >= 1
    assert e.getFitnessScore() == np.finfo(np.float64).max
    # ragged: tiny source (fewer points than k) against a normal target
    tgt2, src2, T = synth.make_pair("VLP-16", 1, downsample=0.4)
    o = O.OracleRegistration(p)
    PC.load_pair(e, o, tgt2, src2[:7])
    PC.check_align(e, o, T, tol_m=1e-4, tol_rad=1e-4)
    e.close()


def test_two_engines_run_concurrently(gicp_case):
    """The odometry and loop-closure engines live in one process and are driven from different threads."""
    import threading
    e, o, tgt, src, T = gicp_case
    p = O.default_params(O.HGS_NDT_OMP)
    p.resolution = 1.0
    e2 = _hip(p)
    e2.setInputTarget(tgt)
    e2.setInputSource(src)
    ref_a = e.align(np.eye(4)).matrix()
    ref_b = e2.align(T).matrix()
    out = {}

    def run(name, eng, guess):
        out[name] = [eng.align(guess).matrix() for _ in range(4)]

    ta = threading.Thread(target=run, args=("a", e, np.eye(4)))
    tb = threading.Thread(target=run, args=("b", e2, T))
    ta.start(), tb.start()
    ta.join(), tb.join()
    assert all(np.array_equal(m, ref_a) for m in out["a"]) and all(np.array_equal(m, ref_b) for m in out["b"])
    e2.close()


def test_batch_rejects_duplicate_candidates_and_foreign_clouds(gicp_case):
    """Every candidate owns its correspondence scratch and every cloud belongs to one engine's stream."""
    e, o, tgt, src, T = gicp_case
    from hdl_graph_slam_amd.registration import HgsError
    c = e.upload(src)
    with pytest.raises(HgsError):
        e.loop_match_batch([c, c], [np.eye(4, dtype=np.float32)] * 2)
    p = O.default_params(O.HGS_FAST_GICP)
    other = _hip(p)
    with pytest.raises(HgsError):
        other.setInputSource(c)            # created by `e`
    other.close()
    rec, best = e.loop_match_batch([c], [np.eye(4, dtype=np.float32)])
    assert len(rec) == 1 and best in (0, -1)
    c.close()


def test_clouds_outlive_their_engine_safely(gicp_case):
    """hgs_destroy orphans the clouds the caller still holds: destroying or using them afterwards is defined —
    hgs_cloud_destroy frees the orphan, everything else rejects it — instead of a use-after-free of the engine."""
    import ctypes as C
    from hdl_graph_slam_amd import _lib as L
    from hdl_graph_slam_amd.registration import HgsError
    e, o, tgt, src, T = gicp_case
    p = O.default_params(O.HGS_FAST_GICP)
    a = _hip(p)
    c = a.upload(src)
    assert c.size == len(src)
    a.close()                                     # engine first ...
    assert L.lib().hgs_cloud_size(c._h) == 0      # ... the cloud is an orphan now
    out = np.zeros(4, np.float32)
    assert L.lib().hgs_cloud_download(c._h, out.ctypes.data_as(C.c_void_p), 16) == L.HGS_ERR_INVALID_ARGUMENT
    with pytest.raises(HgsError):
        e.setInputSource(c)                       # another engine rejects it as well
    c.close()                                     # ... and destroying it afterwards is fine
    e.setInputSource(src)


def test_ndt_edge_cases():
    """Empty / out-of-grid / cell-less / non-finite / one-point NDT inputs: same flags, counts and pose as the oracle."""
    PC.check_ndt_edge_cases(_hip)


def test_ndt_deviation_from_the_serial_sum():
    """The device adds the per-point NDT contributions with an order-independent exact accumulation; ndt_omp adds them serially in
    index order (its result does not depend on the thread count).  This test MEASURES how far that takes a run from the
    upstream-faithful sum — 100 guesses per neighbourhood mode on the HDL-64E 0.2 m-voxel pair, every run to convergence, HIP engine
    against the oracle's serial-sum mode (mode 0) — asserts that no run of the configuration every launch file uses (DIRECT7 at
    resolution 1.0, launch/hdl_graph_slam.launch:81-82) ends more than the north-star tolerance (1e-3 m / 1e-3 rad) away, bounds
    the other modes at 2 %, and leaves the measured fractions in gpurun_out/r03_ndt_serial_sum_deviation.json
    (-> profiles/r03_ndt_sum_mode_deviation.md)."""
    tgt, src, T = synth.make_pair("HDL-64E", 10, downsample=0.2)   # scene seed 10: the pair on which the host fuzz sweep saw prefixes separate
    rows = PC.ndt_serial_sum_deviation(_hip, tgt, src, T, n_guesses=100, seed=10)
    PC.write_report("r03_ndt_serial_sum_deviation.json", {"pair": "HDL-64E scene seed 10, voxel 0.2 m", "points": int(len(src)), "modes": rows})
    for r in rows:
        limit = 0 if r["neighbor_search"] == O.HGS_DIRECT7 else 2
        assert r["beyond_1e-3"] <= limit and r["other_iteration_count"] <= limit, r


def test_nn1_with_equidistant_target_points():
    PC.check_nn1_with_equidistant_targets(_hip)


def test_nn1_on_small_trees():
    PC.check_nn1_on_small_trees(_hip)
