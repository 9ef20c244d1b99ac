"""rgc::NormalEstimationHip (rgc-slam_amd/cpp/features_hip.hpp) on the MI355X: tests/cpp/test_normals.cpp is built the way tests/test_gpu_cpp_plane.py builds its
program and run on designed cases of tests/normal_cases.py -- the k route on a cloud that is its own surface with a viewpoint inside it, and the radius route
against a separate surface with rows of no members; the adaptor's counts and valid rows equal the reference's, its normals, covariances and centroids lie
within the reference's bounds (tests/test_gpu_normals.compare), and its normals and counts equal what the C-ABI gives in the same context, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import normal_cases as nc
from test_gpu_normals import compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("normals") / "test_normals"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_normals.cpp"), "-o", str(out),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    return out


@pytest.mark.parametrize("name,i", [("sheet", 2), ("surface", 1), ("plane", 3)])
def test_the_cpp_adaptor_gives_the_c_abis_and_the_references_result(exe, tmp_path, name, i):
    c = nc.cases()[name]
    r = c["runs"][i]
    c["cloud"].tofile(tmp_path / "cloud.f32")
    if c["surface"] is not None:
        c["surface"].tofile(tmp_path / "surface.f32")
    args = [str(tmp_path / "cloud.f32"), str(tmp_path / "surface.f32") if c["surface"] is not None else "-", str(r["k"]), repr(r["radius"])] + [repr(v) for v in r["vp"]] + [str(int(r["flip"]))]
    run = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-2000:])
    rows = {}
    for line in run.stdout.splitlines():
        f = line.split()
        assert len(f) - 2 == int(f[1])
        rows[f[0]] = np.array(f[2:], np.int32) if f[0] in "MBV" else np.array([float.fromhex(v) for v in f[2:]])
    n = len(c["cloud"])
    n4 = rows["N"].astype(np.float32).reshape(n, 4)
    assert np.array_equal(n4.view(np.uint32), rows["A"].astype(np.float32).reshape(n, 4).view(np.uint32)) and np.array_equal(rows["M"], rows["B"])
    ref = nc.ref(name, i)
    assert rows["V"].tolist() == [ref["n_valid"], ref["n_valid"]]
    got = dict(n4=n4, cov6=rows["S"].reshape(n, 6), cen=rows["D"].reshape(n, 3), cnt=rows["M"], n_valid=int(rows["V"][0]), info=dict(n_valid=int(rows["V"][1])))
    compare(name, i, got)
