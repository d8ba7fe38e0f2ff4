"""adapters/floor_detection_hip.hpp through tests/cpp/floor_adapter_main.cpp (mock PCL / Eigen headers), linked with the library under test, against
the Python mirror on the same library: the same result record and the same coefficients, bit for bit; a prefilter output is found resident."""
import os
import subprocess

import numpy as np

import floor_checks as FC
from hdl_graph_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(lib: str, exe_name: str, link_name: str) -> str:
    exe = os.path.join(ROOT, "tests", "cpp", exe_name)
    src = os.path.join(ROOT, "tests", "cpp", "floor_adapter_main.cpp")
    deps = [src, os.path.join(ROOT, "adapters", "floor_detection_hip.hpp"), os.path.join(ROOT, "adapters", "resident_clouds_hip.hpp"),
            os.path.join(ROOT, "include", "hgs_registration.h"), lib]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "mock_pcl"), "-I", os.path.join(ROOT, "tests", "mock_eigen"), "-I",
                        os.path.join(ROOT, "include"), src, "-o", exe, "-L", os.path.dirname(lib), "-l" + link_name, f"-Wl,-rpath,{os.path.dirname(lib)}"], check=True)
    return exe


def _parse(lines):
    f = lines[0].split()
    rec = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    bits = np.array([int(v, 16) for v in lines[1].split()[1:]], np.uint32)
    sizes = [int(v) for v in lines[2].split()[1:]]
    return rec, bits.view(np.float32), sizes


def _same(rec, co, sizes, d, got):
    r = d.last
    assert rec == {"ran": 1, "detected": r.detected, "reason": r.reason, "clipped": r.n_clipped, "filtered": r.n_filtered, "inliers": r.n_inliers,
                   "iterations": r.ransac_iterations}
    assert co.tobytes() == (np.zeros(4, np.float32) if got is None else got).tobytes()
    assert sizes == [r.n_filtered, r.n_inliers if r.detected else 0]


def check_adapter(make, tmp_path, lib, exe_name, link_name):
    exe = build(lib, exe_name, link_name)
    cloud = FC.scan("vlp16")
    raw = synth.make_pair("VLP-16", 2)[0]
    cloud.tofile(tmp_path / "c.bin")
    raw.tofile(tmp_path / "r.bin")
    for nf, seed in ((1, 0), (0, 3)):
        files = [str(tmp_path / "c.bin")] + ([str(tmp_path / "r.bin")] if nf else [])      # the raw sweep through the prefilter: once
        out = subprocess.run([exe, str(nf), str(seed), *files], check=True, capture_output=True, text=True).stdout.splitlines()
        d = make({"use_normal_filtering": bool(nf)}, seed=seed)
        got = d.detect(cloud)
        assert got is not None
        _same(*_parse(out[0:3]), d, got)
        assert out[3] == "resident_hits 0"
        if not nf:
            d.close()
            continue
        pre = d.engine.prefilter(raw)
        assert out[4] == f"prefiltered {pre.size}"
        got = d.detect(pre)
        _same(*_parse(out[5:8]), d, got)
        assert out[8] == "resident_hits 1"                  # the prefilter's output was taken from the device
        pre.close()
        d.close()
