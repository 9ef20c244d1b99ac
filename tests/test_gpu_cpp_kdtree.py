"""rgc::KdTreeHip (rgc-slam_amd/cpp/kdtree_hip.hpp) on the MI355X: tests/cpp/test_kdtree.cpp is built the way tests/test_cpp_builds.py builds its programs
and run on the lattice case of tests/search_cases.py; the rows it prints -- the single-point and the batched members, sorted and unsorted -- are compared
with the numpy reference for equality (indices, and the keys' bit patterns)."""
import os
import subprocess

import numpy as np
import pytest

import search_cases as sc
import search_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rgc-slam_amd")


def test_the_cpp_adaptor_returns_the_references_rows(tmp_path):
    case = sc.lattice_case()
    tgt, qry = case["tgt"], case["qry"][:400]
    exe = tmp_path / "test_kdtree"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(ROOT, "tests", "cpp", "test_kdtree.cpp"), "-o", str(exe),
                           "-L", PKG, "-lrgc_hip", "-Wl,-rpath," + PKG])
    np.ascontiguousarray(tgt, np.float32).tofile(tmp_path / "cloud.f32")
    np.ascontiguousarray(qry, np.float32).tofile(tmp_path / "queries.f32")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.f32"), str(tmp_path / "queries.f32")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        v = np.array(f[3:], np.int64).reshape(int(f[2]), 2)
        rows[(f[0], int(f[1]))] = (v[:, 0].astype(np.int32), v[:, 1].astype(np.uint32))
    k5, k7 = sr.knn_rows(tgt, qry, 5), sr.knn_rows(tgt, qry[:8], 7)
    off, idx, key = sr.radius_csr(tgt, qry, 0.125, 0)
    off3, idx3, key3 = sr.radius_csr(tgt, qry[:8], 0.125, 3)
    assert sum(t == "K" for t, _ in rows) == len(qry) and sum(t == "R" for t, _ in rows) == len(qry) and sum(t == "U" for t, _ in rows) == len(qry)
    for i in range(len(qry)):
        gi, gb = rows[("K", i)]
        assert np.array_equal(gi, k5[0][i]) and np.array_equal(gb, k5[1][i].view(np.uint32)), ("K", i)
        gi, gb = rows[("R", i)]
        assert np.array_equal(gi, idx[off[i]:off[i + 1]]) and np.array_equal(gb, key[off[i]:off[i + 1]].view(np.uint32)), ("R", i)
        gi, gb = rows[("U", i)]
        o = np.lexsort((gi, gb))        # (non-negative fp32 bit patterns order as the floats do)
        assert np.array_equal(gi[o], idx[off[i]:off[i + 1]]) and np.array_equal(gb[o], key[off[i]:off[i + 1]].view(np.uint32)), ("U", i)
    for i in range(8):
        gi, gb = rows[("k", i)]
        assert np.array_equal(gi, k7[0][i]) and np.array_equal(gb, k7[1][i].view(np.uint32)), ("k", i)
        gi, gb = rows[("r", i)]
        assert np.array_equal(gi, idx3[off3[i]:off3[i + 1]]) and np.array_equal(gb, key3[off3[i]:off3[i + 1]].view(np.uint32)), ("r", i)
