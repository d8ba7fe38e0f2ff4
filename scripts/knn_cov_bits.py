#!/usr/bin/env python3
"""Covariances of fixed clouds under the library in place, for a bit-for-bit comparison of two builds of k_knn_cov on one device.

    python scripts/knn_cov_bits.py dump A.npz        # with the first library in hdl_graph_slam_amd/lib/
    python scripts/knn_cov_bits.py dump B.npz        # with the second one copied into place (a process of its own)
    python scripts/knn_cov_bits.py compare A.npz B.npz

Clouds: two ray-cast HDL-64E scans of scene 3 (~119 k points), parity_checks.tie_heavy_cloud, parity_checks.outlier_cloud.  Per cloud: FROBENIUS at
k = 20, 10 and 48 and PLANE at k = 20 under the engine's own gather; the first scan also with the gather forced to the tree walk and to the leaf-log
replay (engine option knn_replay): 24 covariance arrays.  Every input is stored next to them as its SHA-256 (28 arrays in all), so that `compare` also says when the inputs were not the same.
(profiles/knn_trim_ab_bench.md)"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np


def dump(path):
    import oracle as O
    import parity_checks as PC
    from hdl_graph_slam_amd import synth, _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP

    scene = synth.make_scene(3)
    clouds = {"hdl64": synth.scan(scene, "HDL-64E", synth.pose_matrix([0, 0, 0], [0, 0, 0]), 31),
              "hdl64_b": synth.scan(scene, "HDL-64E", synth.pose_matrix([3, 1, 0], [0, 0, 0.2]), 32),
              "ties": PC.tie_heavy_cloud(), "outliers": PC.outlier_cloud()}
    out = {}
    for name, c in clouds.items():
        out["in_" + name] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(c).tobytes()).digest(), np.uint8)
        for method, k in ((O.HGS_REG_FROBENIUS, 20), (O.HGS_REG_PLANE, 20), (O.HGS_REG_FROBENIUS, 10), (O.HGS_REG_FROBENIUS, 48)):
            for opts in ("", "knn_replay=0", "knn_replay=1"):
                if opts and name != "hdl64":
                    continue
                os.environ["HGS_ENGINE_OPTIONS"] = opts      # read when the engine is created
                p = L.default_params(O.HGS_FAST_GICP)
                p.correspondence_randomness, p.regularization_method = k, method
                e = RegistrationHIP(p)
                e.setInputTarget(c)
                out[f"{name}_{method}_{k}_{opts}"] = e.target_covariances(len(c)).copy()
                e.close()
    np.savez(path, **out)
    print("saved", len(out), "arrays;", {k: len(v) for k, v in clouds.items()})


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = 0
    for k in a.files:
        same = a[k].tobytes() == b[k].tobytes()
        bad += not same
        if not same:
            print(k, "DIFFERS:", int((a[k] != b[k]).sum()), "values of", a[k].size)
    print(f"{len(a.files)} arrays compared, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
