"""rgc::SACSegmentationHip (rgc-slam_amd/cpp/segmentation_hip.hpp) on the MI355X: tests/cpp/test_plane.cpp is built the way tests/test_gpu_cpp_segmentation.py
builds its program and run on two designed cases of tests/plane_cases.py -- `axis_some` (the perpendicular-plane model, invalid positions, caller's samples)
without refinement and `size_1025` with it; the adaptor's segment() gives the reference's inliers, its coefficients and inliers equal what the C-ABI gives
in the same context, bit for bit, and filter() under setNegative(true) gives exactly the other points in input order."""
import os
import subprocess

import numpy as np
import pytest

import plane_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("plane") / "test_plane"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_plane.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    return out


@pytest.mark.parametrize("name,optimize", [("axis_some", 0), ("size_1025", 1)])
def test_the_cpp_adaptor_gives_the_c_abis_and_the_references_result(exe, tmp_path, name, optimize):
    c = pc.case(name)
    prm = c["prm"]
    np.ascontiguousarray(c["cloud"][:, :3], np.float32).tofile(tmp_path / "cloud.f32")
    c["samples"].tofile(tmp_path / "samples.i32")
    args = [str(tmp_path / "cloud.f32"), str(tmp_path / "samples.i32"), repr(prm["threshold"]), str(prm["max_iterations"]), str(optimize), str(prm["seed"]),
            "11" if prm["model"] else "0"] + [repr(v) for v in prm["axis"]] + [repr(prm["eps_angle"])]
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        assert len(f) - 2 == int(f[1])
        rows[f[0]] = np.array(f[2:], np.int32) if f[0] in "IAN" else np.array([float.fromhex(v) for v in f[2:]])
    ref = pc.ref(name, optimize)
    n = len(c["cloud"])
    assert np.array_equal(rows["I"], rows["A"]) and np.array_equal(rows["C"], rows["D"]) and len(rows["C"]) == 4
    assert np.array_equal(rows["N"], np.setdiff1d(np.arange(n), rows["I"]))
    if optimize:
        tol, undecided = pc.tolerances(ref, c["cloud"])
        assert (np.abs(rows["C"] - ref["coeff_exact"]) <= tol).all(), (rows["C"], ref["coeff_exact"], tol)
        if ref["threshold_margin"] > undecided:
            assert np.array_equal(rows["I"], ref["inliers"])
    else:
        assert np.array_equal(rows["I"], ref["inliers"]) and np.array_equal(rows["C"], ref["coeff"])
