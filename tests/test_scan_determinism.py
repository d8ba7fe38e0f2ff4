"""Ray-cast scans do not depend on how many host threads cast them: workloads._cast_scans on several threads returns the sequential loop's arrays bit for
bit (hdl_graph_slam_amd/synth.py keeps its one BLAS product out of concurrent calls, which a threaded BLAS splits differently — a few returns then
cross a range gate and the benchmark's inputs, and with them its outputs, differ from run to run)."""
import numpy as np

from hdl_graph_slam_amd import synth, workloads


def test_threaded_casting_returns_the_sequential_scans(monkeypatch):
    monkeypatch.setenv("HGS_SCAN_CACHE", "")
    scene = synth.make_scene(0)
    jobs = [(synth.pose_matrix([0.7 * j, 0.1 * j, 0.0], [0.0, 0.0, 0.05 * j]), 500 + j) for j in range(8)]
    ref = workloads._cast_scans(scene, "VLP-16", jobs, None, 1)
    for _ in range(2):
        got = workloads._cast_scans(scene, "VLP-16", jobs, None, 8)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ref, got))
    assert len({len(s) for s in ref}) > 1      # the poses give different scans
