"""rgc::StatisticalOutlierRemovalHip / rgc::RadiusOutlierRemovalHip (rgc-slam_amd/cpp/filters_hip.hpp) on the MI355X: tests/cpp/test_filters.cpp is built
the way tests/test_gpu_cpp_kdtree.py builds its program and run on the `mid` case of tests/outlier_cases.py; the kept and removed indices it prints, the mean
distances' bit patterns and the counts are compared with the numpy reference for equality."""
import os
import subprocess

import numpy as np
import pytest

import outlier_cases as oc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")


def test_the_cpp_adaptors_keep_the_references_points(tmp_path):
    case = oc.CASES["mid"]
    cloud, n = case["cloud"], len(case["cloud"])
    mean_k, std_mul = case["sor"][1]
    radius, min_nb = case["ror"][0]
    exe = tmp_path / "test_filters"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_filters.cpp"), "-o", str(exe),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    np.ascontiguousarray(cloud, np.float32).tofile(tmp_path / "cloud.f32")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.f32"), str(mean_k), repr(std_mul), repr(radius), str(min_nb)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows[f[0]] = np.array(f[2:], np.uint32)
        assert len(rows[f[0]]) == int(f[1])
    ref = oc.ref_sor("mid", mean_k, std_mul)
    kept, cnt = np.flatnonzero(ref["inlier"]), oc.ref_counts("mid", radius)
    assert 0 < len(kept) < n
    assert np.array_equal(rows["S"], kept) and np.array_equal(rows["s"], np.flatnonzero(~ref["inlier"])) and np.array_equal(rows["N"], rows["s"])
    assert np.array_equal(rows["D"], ref["d"].view(np.uint32))
    keep_r = cnt - 1 >= min_nb
    assert np.array_equal(rows["R"], np.flatnonzero(keep_r)) and np.array_equal(rows["r"], np.flatnonzero(~keep_r)) and np.array_equal(rows["C"], cnt.view(np.uint32))
