"""What the designed FPFH cases contain and whether the reference can be trusted, without a GPU: every case meets the minima it declares (pairs, swaps,
exact ties, vn == 0, skipped and invalid members, duplicates, isolated points, empty rows, the marked share of a separate surface, the longest rows and
largest counts) as the REFERENCE ALONE finds them; no more than 0.1 % of a case's surface points own an undecided pair -- a condition on the cases, not a
measurement --; the lattice cases own none and their counts are the prototype's; and the vectorised reference equals a literal per-pair Python loop written
from the header's text on a 200-point cloud, count by count, with the descriptors inside each other's bounds."""
import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_reference as fr

CASES = fc.cases()
LD = np.longdouble


@pytest.mark.parametrize("name", list(CASES))
def test_a_case_contains_what_it_declares_and_few_undecided_pairs(name):
    case, ref = CASES[name], fc.ref(name)
    cen, mn = ref["census"], CASES[name]["minima"]
    ns = len(fc.surface_of(case))
    print(name, cen, "n_spfh", ref["n_spfh"], "empty rows", ref["empty_rows"], "largest count", ref["max_count"], "longest row", ref["max_members"], "tainted", int(ref["tainted"].sum()))
    for what in ("pairs", "swaps", "vn0", "ties", "invalid_members", "key0"):
        if what in mn:
            assert cen[what] >= mn[what], (name, what, cen[what])
    assert cen["owners"] <= 0.001 * ns, (name, cen["owners"], ns)
    assert cen["owners"] <= mn.get("undecided_max", ns)
    assert cen["computed"] + cen["vn0"] == cen["pairs"] and cen["skipped"] >= cen["vn0"] + cen.get("key0", 0)
    if "isolated" in mn:
        assert int((ref["spfh_count"] == 1).sum()) >= mn["isolated"] and (ref["spfh"][ref["spfh_count"] == 1] == 0).all()
    if "empty_rows" in mn:
        assert ref["empty_rows"] == mn["empty_rows"] and np.isnan(ref["fpfh"][ref["count"] == 0]).all() and ref["n_valid"] == len(case["cloud"]) - mn["empty_rows"]
    if "n_spfh_max" in mn:
        assert mn["n_spfh_min"] <= ref["n_spfh"] <= mn["n_spfh_max"] < ns and (ref["spfh_count"][~ref["computed"]] == -1).all()
    else:
        assert ref["n_spfh"] == ns and (ref["spfh_count"] >= 1).all()
    for what in ("max_count", "max_members"):
        if what in mn:
            assert ref[what] >= mn[what], (name, what, ref[what])
    v = ~np.isnan(ref["fpfh"][:, 0])
    sums = ref["fpfh"][v].reshape(-1, 3, 11).sum(axis=2)
    assert (np.abs(sums[sums != 0] - 100.0) < 1e-9).all() and (ref["fpfh"][v] >= 0).all()
    assert (ref["spfh"][~ref["valid"]] == 0).all()
    assert (ref["spfh"].reshape(ns, 3, 11).sum(axis=2) == ref["spfh"].reshape(ns, 3, 11).sum(axis=2)[:, :1]).all()      # a pair lands once in every block


def test_the_lattice_counts_are_exact():
    a, b = fc.ref("lattice_16")["census"], fc.ref("lattice_201")["census"]
    assert (a["pairs"], a["vn0"], a["ties"], a["undecided"]) == (7392, 1792, 4032, 0)
    assert (b["pairs"], b["vn0"], b["ties"], b["undecided"]) == (12440, 3328, 7544, 0)


def _literal(P, N, r):
    """the header's text pair by pair, in longdouble scalars: (counts, m, fpfh)"""
    n = len(P)
    r2 = np.float32(np.float64(r) * np.float64(r))
    key = np.zeros((n, n), np.float32)
    for i in range(n):
        for j in range(n):
            d = P[i] - P[j]
            key[i, j] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    member = key < r2
    counts, m = np.zeros((n, 33), np.int64), member.sum(axis=1)
    pi = LD("3.14159265358979323846264338327950288")
    for s in range(n):
        if not np.isfinite(N[s]).all():
            continue
        for t in np.flatnonzero(member[s]):
            if key[s, t] == 0 or not np.isfinite(N[t]).all():
                continue
            a, b = N[s].astype(LD), N[t].astype(LD)
            d = P[t].astype(LD) - P[s].astype(LD)
            f4 = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            c1, c2 = (a[0] * d[0] + a[1] * d[1]) + a[2] * d[2], (b[0] * d[0] + b[1] * d[1]) + b[2] * d[2]
            if abs(c1) < abs(c2):
                u, n2, d, f3 = b, a, -d, -c2 / f4
            else:
                u, n2, f3 = a, b, c1 / f4
            v = np.array([d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]], LD)
            vn = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            if vn == 0:
                continue
            v = v / vn
            w = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], LD)
            f2 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2]
            f1 = np.arctan2((w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2], (u[0] * n2[0] + u[1] * n2[1]) + u[2] * n2[2])
            for blk, x in enumerate(((f1 + pi) * (1 / (2 * pi)), (f2 + 1) * LD(0.5), (f3 + 1) * LD(0.5))):
                counts[s, blk * 11 + min(max(int(np.floor(11 * x)), 0), 10)] += 1
    out = np.zeros((n, 33))
    for q in range(n):
        F = np.zeros(33, LD)
        for j in np.flatnonzero(member[q]):
            if key[q, j] > 0 and np.isfinite(N[j]).all() and m[j] > 1:
                F += (counts[j].astype(LD) * (LD(100) / LD(m[j] - 1))) * (LD(1) / LD(key[q, j]))
        for blk in range(3):
            s = F[blk * 11:blk * 11 + 11].sum()
            if s != 0:
                out[q, blk * 11:blk * 11 + 11] = F[blk * 11:blk * 11 + 11] * (100 / s)
    return counts, m, out


def test_the_reference_equals_a_literal_loop_on_200_points():
    rng = np.random.default_rng(2611)
    P = rng.uniform(-0.3, 0.3, (200, 3)).astype(np.float32)
    P[190:] = P[:10]                                        # duplicates: key 0
    N = rng.normal(0, 1, (200, 3)).astype(np.float32)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[5] = np.nan
    N[17, 1] = np.inf
    ref = fr.estimate(P, N, 0.2)
    counts, m, out = _literal(P, N, 0.2)
    assert ref["census"]["undecided"] == 0 and ref["census"]["pairs"] > 3000 and ref["census"]["key0"] == 20 and ref["census"]["invalid_members"] > 30
    assert np.array_equal(ref["spfh"], counts) and np.array_equal(ref["spfh_count"], m) and np.array_equal(ref["count"], m)
    assert (np.abs(ref["fpfh"] - out) <= ref["bound"]).all() and (ref["fpfh"] > 0).sum() > 3000
