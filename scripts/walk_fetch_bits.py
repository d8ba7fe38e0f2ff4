#!/usr/bin/env python3
"""Results of the 1-NN quad walks (and the covariances) on fixed clouds under the library in place, for a bit-for-bit comparison of two builds on one device.

    python scripts/walk_fetch_bits.py dump A.npz        # with the first library in hdl_graph_slam_amd/lib/
    python scripts/walk_fetch_bits.py dump B.npz        # with the second one copied into place (a process of its own)
    python scripts/walk_fetch_bits.py compare A.npz B.npz

Pairs (target, source): two ray-cast HDL-64E scans of scene 3 (~119 k points each), 8193 points of a 0.25 m grid against a fifth of themselves, and
parity_checks.tie_heavy_cloud against a third of itself.  Per pair: H / b / error / correspondences of hgs_debug_gicp_linearize at a first pose (unseeded)
and at a moved pose (seeded by the first call), hgs_fitness at max_range = max double and 1.0 with its inlier count, hgs_nn_target of the source, and the
target's covariances (FROBENIUS, k = 20).  Every input is stored next to them as its SHA-256, so that `compare` also says when the inputs were not the same.
(profiles/walk_fetch_ab_bench.md)"""
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
    import walk_step_checks as WC
    from hdl_graph_slam_amd import synth, _lib as L
    from hdl_graph_slam_amd.registration import RegistrationHIP

    scene = synth.make_scene(3)
    grid, ties = WC.grid_target(), PC.tie_heavy_cloud()
    pairs = {"hdl64": (synth.scan(scene, "HDL-64E", synth.pose_matrix([0, 0, 0], [0, 0, 0]), 31),
                       synth.scan(scene, "HDL-64E", synth.pose_matrix([3, 1, 0], [0, 0, 0.2]), 32),
                       synth.pose_matrix([2.8, 1.1, 0.0], [0, 0, 0.19]), synth.pose_matrix([2.9, 1.05, 0.0], [0, 0, 0.195])),
             "grid": (grid, grid[::5].copy(), synth.pose_matrix([0.125, 0.0, 0.0], [0, 0, 0]), synth.pose_matrix([0.125, 0.125, 0.0], [0, 0, 0])),
             "ties": (ties, ties[::3].copy(), synth.pose_matrix([0.0, 0.0, 0.0], [0, 0, 0]), synth.pose_matrix([0.125, 0.0, 0.0], [0, 0, 0]))}
    out = {}
    for name, (tgt, src, T0, T1) in pairs.items():
        for tag, c in (("tgt", tgt), ("src", src)):
            out[f"in_{name}_{tag}"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(c).tobytes()).digest(), np.uint8)
        e = RegistrationHIP(L.default_params(O.HGS_FAST_GICP))
        e.setInputTarget(tgt)
        e.setInputSource(src)
        for tag, T in (("unseeded", T0), ("seeded", T1)):
            H, b, err, corr = e.gicp_linearize(T)
            out[f"{name}_{tag}_H"], out[f"{name}_{tag}_b"], out[f"{name}_{tag}_err"], out[f"{name}_{tag}_corr"] = H, b, np.array([err]), corr
        for tag, mr in (("max", float(np.finfo(np.float64).max)), ("1m", 1.0)):
            f = e.getFitnessScore(mr, T=T1)
            out[f"{name}_fitness_{tag}"] = np.array([f, float(e.last_num_inliers)])
        idx, d2 = e.nn_target(src)
        out[f"{name}_nn_idx"], out[f"{name}_nn_d2"] = idx, d2
        out[f"{name}_cov"] = e.target_covariances(len(tgt)).copy()
        e.close()
    np.savez(path, **out)
    print("saved", len(out), "arrays;", {k: (len(v[0]), len(v[1])) for k, v in pairs.items()})


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
