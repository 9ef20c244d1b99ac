"""rgc::EuclideanClusterExtractionHip (rgc-slam_amd/cpp/segmentation_hip.hpp) on the MI355X: tests/cpp/test_segmentation.cpp is built the way
tests/test_gpu_cpp_filters.py builds its program and run on two designed cases of tests/cluster_cases.py -- `limits` under (2, 7), where components are
dropped on both sides and six-fold ties are ordered by leader, and `double_helix`, the near miss; the clusters it prints, in rank order, and the labels are
compared with the numpy / scipy reference for equality."""
import os
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import cluster_reference as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("seg") / "test_segmentation"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_segmentation.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    return out


@pytest.mark.parametrize("name,tol,lo,hi", [("limits", 0.5, 2, 7), ("double_helix", 0.5, 1, cc.INT_MAX)])
def test_the_cpp_adaptor_extracts_the_references_clusters(exe, tmp_path, name, tol, lo, hi):
    cloud = cc.CASES[name]["cloud"]
    np.ascontiguousarray(cloud, np.float32).tofile(tmp_path / "cloud.f32")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.f32"), repr(tol), str(lo), str(hi)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    rows = {"C": []}
    for line in r.stdout.splitlines():
        f = line.split()
        v = np.array(f[2:], np.int32)
        assert len(v) == int(f[1])
        if f[0] == "C":
            rows["C"].append(v)
        else:
            rows[f[0]] = v
    ref = cc.ref(name, tol, lo, hi)
    want = cr.rows(ref)
    assert rows["M"][0] == len(rows["C"]) == ref["n_clusters"] > 1
    assert all(np.array_equal(a, b) for a, b in zip(rows["C"], want)) and np.array_equal(rows["L"], ref["labels"])
