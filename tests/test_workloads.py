"""hdl_graph_slam_amd/workloads.py: the seeded workloads do not depend on how many host threads ray-cast their scans."""
import numpy as np

from hdl_graph_slam_amd import synth, workloads


def test_loop_closure_set_is_the_same_for_every_worker_count(monkeypatch):
    monkeypatch.setenv("HGS_SCAN_CACHE", "")
    one = workloads.make_loop_closure_set("VLP-16", scene_seed=2, n_candidates=5, n_distinct=3, downsample=0.4)
    many = workloads.make_loop_closure_set("VLP-16", scene_seed=2, n_candidates=5, n_distinct=3, downsample=0.4, workers=4)
    assert np.array_equal(one.target, many.target) and len(one.candidates) == len(many.candidates) == 5
    for a, b in zip(one.candidates + one.T_gt + one.guesses, many.candidates + many.T_gt + many.guesses):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    # the scans draw nothing from the generator of the poses and guesses: a scan cast between two pose draws (the order a sequential
    # caller sees) is the scan of the set
    rng = np.random.default_rng(7000 + 2)
    scene = synth.make_scene(2)
    for j in range(3):
        xy = rng.uniform(-20.0, 20.0, 2)
        xy[1] *= 0.3 * min(1.0, 4.0 / 20.0)
        pose = synth.pose_matrix([xy[0], xy[1], 0.0], np.deg2rad([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-8, 8)]))
        sc = synth.voxel_downsample(synth.scan(scene, "VLP-16", pose, 3000 + 17 * 2 + j), 0.4)
        assert np.array_equal(sc, many.candidates[j])
        assert np.array_equal(pose, many.T_gt[j])   # the query sits at the origin


def test_odometry_stream_is_the_same_for_every_worker_count(monkeypatch):
    monkeypatch.setenv("HGS_SCAN_CACHE", "")
    one = workloads.make_odometry_stream("VLP-16", 1, 4, speed=2.0, downsample=0.4)
    many = workloads.make_odometry_stream("VLP-16", 1, 4, speed=2.0, downsample=0.4, workers=3)
    assert one.stamps == many.stamps and len(many.scans) == 4
    for a, b in zip(one.scans + one.poses, many.scans + many.poses):
        assert np.array_equal(a, b)
