"""The normal-estimation reference (tests/normal_reference.py) and the designed cases (tests/normal_cases.py) on the CPU, after tests/test_plane_reference.py: every
minimum a case declares holds from the reference alone, the reference's rows equal a brute-force all-pairs search on the small cases, its bounds are sane, and a
literal restatement of PCL's fp32 unshifted computePointNormal agrees with the reference in direction on the sheet near the origin, within its own fp32 bound,
and visibly fails on the same sheet translated by (1000, -2000, 500): the deviation the header lists, demonstrated."""
import numpy as np
import pytest

import knn_reference as kr
import normal_cases as nc
import normal_reference as nr
import search_reference as sr

CASES = nc.cases()


def test_the_declared_minima_hold_from_the_reference_alone():
    for name, c in CASES.items():
        mi = c["minima"]
        for i, r in enumerate(c["runs"]):
            ref = nc.ref(name, i)
            v = ref["valid"]
            assert len(ref["count"]) == len(c["cloud"]) and ref["n_valid"] == int(v.sum())
            assert np.isfinite(ref["cov6"][v]).all() and (ref["bound_cov"][v] >= 0).all() and (ref["bound_n"][ref["decided"]] < 1e-3).all(), (name, i)
            if mi.get("all_decided"):
                assert ref["decided"].all() and ref["gap_rel"].min() >= mi["min_gap"], (name, i, ref["gap_rel"].min())
            if "nan_rows" in mi and r["radius"]:
                assert int((~v).sum()) == mi["nan_rows"][r["radius"]], (name, r["radius"], int((~v).sum()))
            if "max_undecided" in mi:
                und = int((v & ~ref["decided"]).sum())
                assert und <= mi["max_undecided"] * int(v.sum()), (name, i, und, int(v.sum()))
                if r["k"]:
                    assert v.all()
            if "n" in mi:
                assert len(c["cloud"]) == mi["n"]
            if "rank" in mi:
                assert v.all() and (np.sum(ref["ev"] > 2 * kr.GAP_MIN * ref["trace"][:, None], axis=1) <= mi["rank"]).all(), (name, i)
                if mi["rank"] == 0:
                    assert (ref["cov6"] == 0).all()
            if mi.get("all_nan"):
                assert (ref["count"] == 1).all() and ref["n_valid"] == 0
            if "min_members" in mi:
                assert ref["count"].min() >= mi["min_members"]
            if "empty_rows" in mi and r["radius"]:
                assert int((ref["count"] == 0).sum()) == mi["empty_rows"]
            if mi.get("exact_plane"):
                assert (ref["cov6"][v][:, [2, 4, 5]] == 0).all()               # xz, yz, zz: the sheet is exactly planar in the reference's arithmetic too
                assert ref["decided"].sum() >= 0.9 * len(v) and (np.abs(ref["normal"][ref["decided"], 2]) == 1).all()
    c = CASES["surface"]
    s = c["surface"]
    assert int(((c["cloud"] < s.min(0)) | (c["cloud"] > s.max(0))).any(axis=1).sum()) >= c["minima"]["outside"] + c["minima"]["empty_rows"]
    # lattice: the k-th place is inside an exact tie for every query (ranks 1..6 and 7..18 of an interior point tie; border points have ties of their own)
    lat = CASES["lattice"]
    for k in (5, 10):
        _, key = sr.knn_rows(lat["cloud"], lat["cloud"], k + 1)
        assert int((key[:, k - 1] == key[:, k]).sum()) >= lat["minima"]["tied_rows"], k
    # lattice at r = the spacing exactly: the six neighbours lie ON the radius and are excluded
    assert (nc.ref("lattice", 2)["count"] == 1).all() and (nc.ref("lattice", 3)["count"] > 1).all()
    # walls: points exactly on cell walls of 0.5
    w = CASES["walls"]["cloud"].astype(np.float64)
    assert int((np.abs(w / 0.5 - 0.5 - np.round(w / 0.5 - 0.5)) == 0).all(axis=1).sum()) >= 100
    # sparse: the strays' tenth neighbour is tens of metres away
    sp = nc.ref("sparse", 0)
    assert int((np.sqrt(np.abs(sp["cov6"][:, 0] + sp["cov6"][:, 3])) > 5).sum()) >= CASES["sparse"]["minima"]["grown"]


@pytest.mark.parametrize("name", ["lattice", "dups", "pole", "n_3", "short_5", "full_8", "tiers", "n_65", "ball", "walls"])
def test_the_rows_equal_brute_force(name):
    c = CASES[name]
    T = nc.surface_of(c)
    for i, r in enumerate(c["runs"]):
        ref = nc.ref(name, i)
        if r["k"]:
            m = min(r["k"], len(T))
            idx, _ = sr.brute_knn(T, c["cloud"], m)
            assert np.array_equal(ref["idx"].reshape(len(c["cloud"]), m), idx)
        else:
            off, idx, _ = sr.brute_radius(T, c["cloud"], r["radius"])
            assert np.array_equal(ref["off"], off) and np.array_equal(ref["idx"], idx)


def test_the_moments_equal_the_mean_centred_definition():
    """cov about the query minus mean mean^T is the mean-centred second moment (knn_reference.sample_covariances) to rounding"""
    c = CASES["sheet_far"]
    ref = nc.ref("sheet_far", 0)
    S = kr.sample_covariances(c["cloud"], ref["idx"].reshape(len(c["cloud"]), 12))
    assert np.abs(S - ref["S"]).max() <= 1e-12 * np.abs(S).max()
    assert np.abs(ref["centroid"] - c["cloud"][ref["idx"].reshape(-1, 12)].astype(np.float64).mean(axis=1)).max() <= 1e-9


def test_pcls_fp32_unshifted_sums_agree_near_the_origin_and_fail_far_from_it():
    rows = np.arange(0, 4000, 20)                                    # 200 queries of each sheet
    worst = {}
    for name in ("sheet", "sheet_far"):
        c = CASES[name]
        ref = nc.ref(name, 0)
        off = np.arange(len(rows) + 1) * 12
        idx = ref["idx"].reshape(-1, 12)[rows].reshape(-1)
        got = nr.pcl_point_normal(c["cloud"][rows], c["cloud"], off, idx)
        cos = np.abs((got * ref["normal"][rows]).sum(axis=1))
        worst[name] = float(np.sqrt(np.maximum(0.0, 1.0 - cos * cos)).max())   # the sine of the angle to the reference's normal
        # the fp32 sums' own bound: m 2^-24 |p|^2 of absolute error in an entry of the covariance, through the eigenvector's condition, times 8
        P = c["cloud"][ref["idx"].reshape(-1, 12)[rows]].astype(np.float64)
        own = 8.0 * 12 * 2.0 ** -24 * (P ** 2).sum(axis=2).max(axis=1) / (ref["ev"][rows, 1] - ref["ev"][rows, 0])
        print(name, "largest sine of the angle between PCL's fp32 normal and the reference's:", worst[name], "its own bound at worst", float(own.max()))
        if name == "sheet":
            assert (np.sqrt(np.maximum(0.0, 1.0 - cos * cos)) <= own).all()
    assert worst["sheet"] < 1e-2 and worst["sheet_far"] > 0.1, worst
