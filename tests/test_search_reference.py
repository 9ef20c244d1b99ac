"""The search index's reference and designed cases, on the CPU alone: every case of tests/search_cases.py meets the minima it declares (so the GPU
tests are known to exercise ties at the k-th place and at the max_nn cut, members on the gate, empty rows, every row-length class about the sort
window, queries outside the box and cubes that must grow), and the wrappers of tests/search_reference.py equal a brute force over every pair on the
small cases -- the reference stays within its own conditions on these inputs before a GPU sees them."""
import numpy as np
import pytest

import search_cases as sc
import search_reference as sr


@pytest.mark.parametrize("case", sc.all_cases(), ids=lambda c: c["name"])
def test_every_case_meets_its_minima(case):
    got = sr.census(case["tgt"], case["qry"], case["ks"], case["radii"], case.get("window", sc.DEFAULT_WINDOW))
    print(case["name"], got)
    for name, least in case["minima"].items():
        assert got[name] >= least, (case["name"], name, got[name], least)
    if "grow" in case:
        k, cell, least = case["grow"]
        must, cannot = sr.grow_census(case["tgt"], case["qry"], k, cell)
        print(case["name"], "k", k, "cell", cell, "must grow", must, "cannot", cannot)
        assert must >= least and must + cannot <= len(case["qry"])


@pytest.mark.parametrize("case", sc.small_cases(), ids=lambda c: c["name"])
def test_the_wrappers_equal_the_brute_force(case):
    for k in case["ks"]:
        idx, key = sr.knn_rows(case["tgt"], case["qry"], k)
        bidx, bkey = sr.brute_knn(case["tgt"], case["qry"], k)
        assert idx.dtype == np.int32 and key.dtype == np.float32 and idx.shape == (len(case["qry"]), k)
        assert np.array_equal(idx, bidx) and np.array_equal(key.view(np.uint32), bkey.view(np.uint32)), (case["name"], k)
    for r, max_nn in case["radii"]:
        got, want = sr.radius_csr(case["tgt"], case["qry"], r, max_nn), sr.brute_radius(case["tgt"], case["qry"], r, max_nn)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w), (case["name"], r, max_nn)


def test_the_sentinel_form_and_the_cut():
    t = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    q = np.array([[0, 0, 0]], np.float32)
    idx, key = sr.knn_rows(t, q, 6)
    assert idx.tolist() == [[0, 1, 2, 3, -1, -1]] and key[0, :4].tolist() == [0, 1, 1, 9] and np.isinf(key[0, 4:]).all()
    off, idx, key = sr.radius_csr(t, q, 3.0, 0)       # key == r2 = 9 is no member
    assert off.tolist() == [0, 3] and idx.tolist() == [0, 1, 2]
    off, idx, key = sr.radius_csr(t, q, 3.0, 2)       # the cut falls between two equal keys: the smaller index stays
    assert off.tolist() == [0, 2] and idx.tolist() == [0, 1] and key.tolist() == [0, 1]
    row, i, k = sr.as_sets(np.array([0, 3]), np.array([2, 0, 1]), np.array([1, 0, 1], np.float32))
    assert i.tolist() == [0, 1, 2]
