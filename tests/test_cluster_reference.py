"""The clustering reference (tests/cluster_reference.py) against a literal restatement of PCL's algorithm, and what the designed cases
(tests/cluster_cases.py) contain, on the CPU: the GPU tests (tests/test_gpu_cluster.py) then compare the product with this reference for equality.  That
the component route and PCL's seed-and-queue route agree on every small case, at every tolerance and every pair of limits, is the proof that "a
connected component" is what PCL computes."""
import numpy as np
import pytest

import cluster_cases as cc
import cluster_reference as cr

SMALL = sorted(n for n, c in cc.CASES.items() if c["small"])


@pytest.mark.parametrize("name", SMALL)
def test_the_components_are_pcls_clusters(name):
    case = cc.CASES[name]
    for tol in case["tol"]:
        for lo, hi in case["limits"]:
            want = cr.pcl_extract(case["cloud"], tol, lo, hi)
            res = cc.ref(name, tol, lo, hi)
            got = cr.rows(res)
            assert len(got) == len(want) == res["n_clusters"], (name, tol, lo, hi)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, tol, lo, hi)
            lab = np.full(len(case["cloud"]), -1, np.int32)
            for r, row in enumerate(want):
                lab[row] = r
            assert np.array_equal(lab, res["labels"])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_the_minima_hold(name):
    case = cc.CASES[name]
    res = cc.ref(name, case["tol"][0], *case["limits"][0])
    print(name, {k: res[k] for k in ("n", "n_components", "n_clusters", "n_clustered", "largest", "edges", "ties", "over", "under", "at_r2", "one_under")})
    for k, want in case["minima"].items():
        assert res[k] >= want, (name, k, res[k], want)
    assert res["n_clustered"] == res["offsets"][-1] == len(res["indices"]) and int((res["labels"] >= 0).sum()) == res["n_clustered"]
    sizes = np.diff(res["offsets"])
    assert (sizes[:-1] >= sizes[1:]).all()
    lead = np.array([row[0] for row in cr.rows(res)], np.int64)
    assert all((np.diff(row) > 0).all() for row in cr.rows(res)) and ((sizes[:-1] > sizes[1:]) | (lead[:-1] < lead[1:])).all()


def test_the_limits_drop_whole_components():
    case = cc.CASES["limits"]
    full = cc.ref("limits", 0.5)
    assert sorted(np.diff(full["offsets"]).tolist()) == sorted(s for s in range(1, 9) for _ in range(6))
    for (lo, hi), kept, over, under in zip(cc.LIMITS, (48, 6, 36, 6, 0), (0, 30, 6, 0, 0), (0, 12, 6, 42, 48)):
        res = cc.ref("limits", 0.5, lo, hi)
        assert (res["n_clusters"], res["over"], res["under"]) == (kept, over, under), (lo, hi)
        size_of = np.diff(full["offsets"])[full["labels"]]
        assert np.array_equal(res["labels"] >= 0, (size_of >= lo) & (size_of <= hi)), "a dropped component's points are in no row"
    assert len(case["cloud"]) == 216


def test_the_near_miss_stays_two_clusters_and_the_tie_is_decided_by_the_leader():
    for tol in cc.CASES["double_helix"]["tol"]:
        res = cc.ref("double_helix", tol)
        assert res["n_clusters"] == 2 and np.diff(res["offsets"]).tolist() == [256, 256] and res["indices"][0] == 0
    cloud = cc.CASES["double_helix"]["cloud"]
    lab = cc.ref("double_helix", 0.5)["labels"]
    assert np.array_equal(cloud[lab == 0].min(0), cloud[lab == 1].min(0)) and np.array_equal(cloud[lab == 0].max(0), cloud[lab == 1].max(0))
