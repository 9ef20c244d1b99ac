"""The outlier filters' reference (tests/outlier_reference.py) against brute force, and what the designed cases (tests/outlier_cases.py) contain, on the
CPU: the GPU tests (tests/test_gpu_outlier.py) then compare the product with this reference point by point.  For every SOR setting of every case NO mean
distance lies within the derived bound of the reference threshold (the cap on undecided points is zero), so the reference's inlier mask is the one
correct answer."""
import numpy as np
import pytest

import outlier_cases as oc
import outlier_reference as orf
import search_reference as sr

SMALL = {c["name"]: c for c in oc.small_cases()}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_reference_equals_brute_force(name):
    case = SMALL[name]
    for mean_k, std_mul in case["sor"]:
        d = oc.ref_sor(name, mean_k, std_mul)["d"]
        assert d.dtype == np.float32 and np.array_equal(d.view(np.uint32), orf.brute_mean_distances(case["cloud"], mean_k).view(np.uint32)), (name, mean_k)
    for radius, _ in case["ror"]:
        assert np.array_equal(oc.ref_counts(name, radius), orf.brute_counts(case["cloud"], radius)), (name, radius)


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_no_point_is_undecided_and_the_minima_hold(name):
    case = oc.CASES[name]
    n = len(case["cloud"])
    for mean_k, std_mul in case["sor"]:
        r = oc.ref_sor(name, mean_k, std_mul)
        print(name, "mean_k", mean_k, "threshold", float(r["threshold"]), "bound", r["bound"], "nearest d", r["min_gap"], "kept", int(r["inlier"].sum()), "of", n)
        assert r["undecided"] == 0 and (r["bound"] == 0.0 or r["min_gap"] > r["bound"]), (name, mean_k, std_mul, r["bound"], r["min_gap"])
        assert r["bound"] <= 1e-9 * max(float(r["threshold"]), 1e-30) + 1e-300, "the bound is a rounding bound, far below any d"
    m = case["minima"]
    for radius, want in m.get("count_1", {}).items():
        assert int((oc.ref_counts(name, radius) == 1).sum()) >= want
    for radius, (min_nb, on, under) in m.get("on_gate", {}).items():
        cnt = oc.ref_counts(name, radius)
        assert int((cnt - 1 == min_nb).sum()) >= on and int((cnt - 1 == min_nb - 1).sum()) >= under
        assert any(r == radius and k == min_nb for r, k in case["ror"])
    if "tied_rows" in m:      # rows whose last kept rank ties with the next one: the choice among equal keys must not matter
        mean_k = case["sor"][0][0]
        _, key = sr.knn_rows(case["cloud"], case["cloud"], mean_k + 2)
        assert int((key[:, mean_k] == key[:, mean_k - 1]).sum() + (key[:, mean_k + 1] == key[:, mean_k]).sum()) >= m["tied_rows"]
    if "zero_ranks" in m:
        _, key = sr.knn_rows(case["cloud"], case["cloud"], 1 + m["zero_ranks"])
        assert (key == 0).all()
    if "strays_removed" in m:
        r = oc.ref_sor(name, *case["sor"][0])
        assert case["sor"][0][1] == 1.0 and len(case["strays"]) == m["strays_removed"] and not r["inlier"][case["strays"]].any()
        assert int((oc.ref_counts(name, case["ror"][0][0])[case["strays"]] == 1).sum()) == m["stray_count_1"]
    if m.get("exact"):
        r = oc.ref_sor(name, *case["sor"][0])
        assert r["bound"] == 0.0 and (r["d"].astype(np.longdouble) == r["threshold"]).all() and r["inlier"].all()
    if "stat_rows" in m:
        assert (n + 255) // 256 >= m["stat_rows"] > 64


def test_the_bound_follows_n_and_vanishes_only_in_the_exact_case():
    rng = np.random.default_rng(5)
    d = rng.uniform(0.1, 0.2, 1000).astype(np.float32)
    b1, b2 = orf.threshold_bound(d[:100], 1.0), orf.threshold_bound(d, 1.0)
    assert 0 < b1 < b2 < 1e-12
    same = np.full(16, 0.3, np.float32)
    assert orf.threshold_bound(same, 1.0) == 0.0 and orf.threshold_bound(np.full(12, 0.3, np.float32), 1.0) > 0
    st = orf.statistics(same, 2.0)
    assert st["threshold"] == np.longdouble(np.float32(0.3)) and st["stddev"] == 0
