#!/usr/bin/env python3
"""What the base_link transform costs a prefilter call on one GPU; prints one JSON line.  Input: one raw HDL-64E sweep (synth.make_pair("HDL-64E", 0)),
the nodelet's default parameters.  One process, three series taken in turn — hgs_prefilter (a), hgs_prefilter_framed with a matrix, hgs_prefilter (b) —
host call to host return, --reps calls each (the returned cloud is released outside the timed region):
  * p50_ms of each series;
  * spread_ms = |p50(a) - p50(b)|: what two series of the SAME call differ by in this run, the yardstick for framed_minus_prefilter_ms
    (= p50(framed) - mean of the two);
  * the matrix is the IDENTITY by default: the kernel does the same arithmetic for it as for any other matrix and the stages behind it get the very points
    hgs_prefilter gives them, so the difference is the transform's own cost; --matrix mounted takes a sensor mount instead (1.9 m up, pitched, yawed),
    after which the filters keep a slightly different number of points (points_out); --matrix none passes NULL — the same launches as hgs_prefilter through
    the new entry point: what the middle place in the turn costs by itself;
  * with --deskew the three series carry a gyro sample as well (hgs_prefilter_deskewed / hgs_prefilter_framed with both)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hdl_graph_slam_amd import synth, _lib as L  # noqa: E402
from hdl_graph_slam_amd.registrations import select_registration_method  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--deskew", action="store_true")
    ap.add_argument("--matrix", default="identity", choices=["identity", "mounted", "none"])
    a = ap.parse_args()
    raw = synth.make_pair("HDL-64E", 0)[0]
    reg = select_registration_method({"registration_method": "FAST_GICP"})
    lib = L.lib()
    pp = L.HgsPrefilterParams()
    lib.hgs_prefilter_params_default(C.byref(pp))
    arr, n, stride = L.cloud_args(raw)
    pts = arr.ctypes.data_as(C.c_void_p)
    # mounted: a sensor 1.9 m above base_link, pitched by 2 degrees and yawed by 30
    T = synth.pose_matrix([0.4, -0.1, 1.9], np.deg2rad([0.0, 2.0, 30.0])) if a.matrix == "mounted" else np.eye(4)
    m = L.colmajor16(T)
    mp = None if a.matrix == "none" else L.fptr(m)
    w = np.array([0.02, -0.01, 0.4], np.float64)
    wp = w.ctypes.data_as(C.c_void_p) if a.deskew else None

    def plain():
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.hgs_prefilter_deskewed(reg._h, pts, n, stride, C.byref(pp), wp, 0.1, C.byref(h)) if a.deskew else lib.hgs_prefilter(reg._h, pts, n, stride, C.byref(pp), C.byref(h))
        dt = (time.perf_counter() - t0) * 1e3
        reg._check(rc)
        size = int(lib.hgs_cloud_size(h))
        lib.hgs_cloud_destroy(h)
        return dt, size

    def framed():
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.hgs_prefilter_framed(reg._h, pts, n, stride, C.byref(pp), wp, 0.1, mp, C.byref(h))
        dt = (time.perf_counter() - t0) * 1e3
        reg._check(rc)
        size = int(lib.hgs_cloud_size(h))
        lib.hgs_cloud_destroy(h)
        return dt, size

    series = {"prefilter_a": [], "framed": [], "prefilter_b": []}
    sizes = {}
    for rep in range(a.warmup + a.reps):
        for name, call in (("prefilter_a", plain), ("framed", framed), ("prefilter_b", plain)):
            dt, sizes[name] = call()
            if rep >= a.warmup:
                series[name].append(dt)
    p50 = {k: float(np.percentile(v, 50)) for k, v in series.items()}
    out = {"raw_points": int(n), "deskew": bool(a.deskew), "matrix": a.matrix, "calls_per_series": a.reps, "points_out": sizes,
           "p50_ms": {k: round(v, 4) for k, v in p50.items()},
           "p10_ms": {k: round(float(np.percentile(v, 10)), 4) for k, v in series.items()},
           "p90_ms": {k: round(float(np.percentile(v, 90)), 4) for k, v in series.items()},
           "spread_ms": round(abs(p50["prefilter_a"] - p50["prefilter_b"]), 4),
           "framed_minus_prefilter_ms": round(p50["framed"] - 0.5 * (p50["prefilter_a"] + p50["prefilter_b"]), 4)}
    reg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
