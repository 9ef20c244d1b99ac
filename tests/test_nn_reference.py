"""The C oracle against tests/nn_reference.py (numpy / scipy, nothing from oracle/), without a GPU: a disagreement about a formula --
the tie rule, the gate, the order of the fp32 transform, the convergence criteria -- is found here and not on the GPU.  The same cases
(tests/nn_cases.py) are what test_gpu_nearest.py hands to the kernels; their census conditions are checked here too."""
import numpy as np
import pytest

import nn_cases as nc
import nn_reference as nnr


@pytest.fixture(scope="module")
def lattice_cases():
    return nc.fitness_lattice_cases()


def _fitness(orc, tgt, src, T):
    o = orc.Registration(num_threads=0)
    o.set_target(tgt)
    o.set_source(src)
    return o.fitness(T)


def test_knn_query_rows_and_keys_bit_for_bit(orc):
    rng = np.random.default_rng(0)
    Is, It = nc.icp_tie_case()
    cases = [(nnr.lattice(It), nnr.lattice(Is)),                                        # hundreds of exact ties
             (rng.normal(0, 5, (6000, 3)).astype(np.float32), rng.normal(0, 7, (3000, 3)).astype(np.float32)),
             (rng.uniform(-1, 1, (7, 3)).astype(np.float32), rng.uniform(-30, 30, (500, 3)).astype(np.float32))]
    for tgt, q in cases:
        for k in (1, 5):
            io, do = orc.knn_query(tgt, q, k)
            ir, dr = nnr.nearest_k(tgt, q, k)
            assert np.array_equal(io, ir) and np.array_equal(do.view(np.uint32), dr.view(np.uint32))


def test_fitness_bit_for_bit_on_lattice_cases(orc, lattice_cases):
    for c in lattice_cases:
        ref = nnr.lattice_score(c["It"], nc.moved(c["Iq"], c["R"], c["t"]))
        tgt, src = nnr.lattice(c["It"]), nnr.lattice(c["Iq"])
        assert _fitness(orc, tgt, src, c["T"]) == ref, c["name"]
        assert nnr.score(tgt, src, c["T"]) == ref, c["name"]                            # the two references agree with each other
        mv = nnr.lattice(nc.moved(c["Iq"], c["R"], c["t"]))
        for res in c["census_res"]:
            cen = nnr.census(tgt, mv, res)
            for cls, least in c["need"].items():
                assert cen[cls] >= least, f"{c['name']} at cell size {res}: {cen}, needs {cls} >= {least}"


def test_tail_case_has_the_cell_populations(lattice_cases):
    c = next(c for c in lattice_cases if c["name"] == "cell_population_tails")
    assert set(nnr.cell_histogram(nnr.lattice(c["It"]), 1.0).tolist()) == set(nc.TAIL_POPULATIONS)


def test_fitness_non_lattice_within_reordering_bound(orc):
    rng = np.random.default_rng(1)
    import rgc_slam_amd.synth as synth
    T = synth.se3(synth.rot_zyx(0.3, -0.1, 0.05), [0.4, -0.2, 0.1]).astype(np.float32)
    tgt = rng.normal(0, 6, (20000, 3)).astype(np.float32)
    src = rng.normal(0, 7, (5000, 3)).astype(np.float32)
    a, b = _fitness(orc, tgt, src, T), nnr.score(tgt, src, T)
    assert abs(a - b) <= nnr.sum_reorder_bound(len(src)) * b
    for res in (0.3, 0.7, 1.9, 3.0):
        t, s = nc.wall_ulp_case(res)
        a, b = _fitness(orc, t, s, np.eye(4, dtype=np.float32)), nnr.score(t, s)
        assert abs(a - b) <= nnr.sum_reorder_bound(len(s)) * b, res
        u = t[:, 0].astype(np.float64) / res - 0.5
        assert (np.abs(u - np.round(u)) * res <= 1.5 * np.spacing(np.abs(t[:, 0]))).all()   # the target really sits on the walls


def test_small_map_cases_hold_what_they_say():
    for nt in (511, 32768):
        for frac in nc.FAR_FRACTIONS:
            It, Iq = nc.small_map_case(nt, frac, 3000)
            assert len(It) == nt and len(np.unique(It, axis=0)) == nt
            cen = nnr.census(nnr.lattice(It), nnr.lattice(Iq), 1.0)
            assert abs(cen["far"] - frac * 3000) <= 1 and cen["outside"] == 0, (nt, frac, cen)


def _lattice_icp_cases():
    out = [(f"gate_{g}", *nc.icp_gate_case(g), g) for g in nc.ICP_GATES]
    out.append(("ties", *nc.icp_tie_case(), 2.0))
    for n in (2, 3):
        out.append((f"kept_{n}", *nc.icp_few_case(n)))
    out.append(("planar", *nc.icp_degenerate_case("planar")))
    out.append(("collinear", *nc.icp_degenerate_case("collinear")))
    return out


def test_icp_first_iteration_matches_oracle(orc):
    for name, Is, It, gate in _lattice_icp_cases():
        src, tgt = nnr.lattice(Is), nnr.lattice(It)
        ref = nnr.icp_first_iteration(src, tgt, gate)
        To, ro = orc.icp_align(src, tgt, max_corr_dist=gate, max_iterations=1)
        assert (ro["n_correspondences"], ro["state"], ro["iterations"]) == (ref["n"], ref["state"], ref["iterations"]), name
        if ref["n"] >= 3:
            nnr.check_rigid(To, ref, src, tgt)
        if name != "collinear":                                                         # Kabsch is not unique on a line
            assert np.abs(To - ref["T"]).max() <= nnr.t_tolerance(ref["T"]), name
        fit = nnr.score(tgt, src, To)
        assert abs(ro["fitness"] - fit) <= nnr.sum_reorder_bound(len(src)) * fit, name
        # what the cases' names say
        cen = nnr.census(tgt, src, 1.0, gate)
        if name.startswith("gate_"):
            assert cen["beyond_gate"] >= 6 * len(It), (name, cen)
            assert cen["on_gate"] >= (6 * len(It) if gate != 0.3 else 0) and (gate != 0.3 or cen["on_gate"] == 0), (name, cen)
        if name == "ties":
            _, k2 = nnr.nearest_k(tgt, src, 2)
            assert int((k2[:, 0] == k2[:, 1]).sum()) >= 300
            # "smaller original index" is not "first in cell order": in a cell-sorted target the other candidate would win for many
            i2, _ = nnr.nearest_k(tgt, src, 2)
            tie = k2[:, 0] == k2[:, 1]
            order = np.lexsort((It[:, 0], It[:, 1], It[:, 2]))
            rank = np.empty(len(It), np.int64); rank[order] = np.arange(len(It))
            assert int((rank[i2[tie, 0]] > rank[i2[tie, 1]]).sum()) >= 100
        if name.startswith("kept_"):
            assert ref["n"] == int(name[-1]) and cen["beyond_gate"] >= 400
        if name in ("planar", "collinear"):
            assert ref["singular"][2] < 1e-9 * ref["singular"][0] and (name == "planar") == (ref["singular"][1] > 1e-3 * ref["singular"][0])


def test_a_single_wrong_correspondence_moves_T():
    """The mutation check: one correspondence of the reference swapped for that query's second candidate (40 sampled kept queries per
    case) must move T by at least 50 times the 4-ulp tolerance, or the tolerance would not see a single wrong neighbour.
    Measured (printed with -s): the smallest change over all cases is 1.15e-4 = 240 x the tolerance, on the tie case (2 134 kept
    correspondences, the second candidate exactly as near as the first); 2.5e-4 = 517 x on the gate cases with 3 888 kept."""
    rng = np.random.default_rng(9)
    worst = np.inf
    for name, Is, It, gate in _lattice_icp_cases():
        if name in ("collinear", "kept_2"):
            continue
        src, tgt = nnr.lattice(Is), nnr.lattice(It)
        ref = nnr.icp_first_iteration(src, tgt, gate)
        i2, _ = nnr.nearest_k(tgt, src, 2)
        kept = np.nonzero(ref["keep"])[0]
        p = src[kept].astype(np.float64)
        q0 = tgt[ref["idx"][kept]].astype(np.float64)
        tol = nnr.t_tolerance(ref["T"])
        least = np.inf
        for j in rng.choice(len(kept), min(40, len(kept)), replace=False):
            q = q0.copy()
            q[j] = tgt[i2[kept[j], 1]]
            R, t, _ = nnr.kabsch(p, q)
            least = min(least, float(np.abs(nnr._T32(R, t).astype(np.float64) - ref["T"]).max()))
        print(f"mutation check {name}: n = {len(kept)}, smallest change of T = {least:.3e} = {least / tol:.0f} x tolerance")
        assert least >= 50 * tol, f"{name}: a single wrong correspondence moves T by only {least:.3e} ({least / tol:.1f} x the tolerance)"
        worst = min(worst, least / tol)
    print(f"mutation check: smallest change over all cases = {worst:.0f} x the 4-ulp tolerance")


def test_icp_full_loop_matches_oracle(orc):
    for c in nc.icp_loop_cases():
        To, ro = orc.icp_align(c["src"], c["tgt"], max_corr_dist=c["gate"])
        Tr, rr = nnr.icp_align(c["src"], c["tgt"], gate=c["gate"])
        assert (ro["iterations"], ro["state"], ro["n_correspondences"]) == (rr["iterations"], rr["state"], rr["n_correspondences"]), \
            f"{c['name']}: oracle {ro}, reference {rr}"
        assert ro["converged"] == 1 and 2 <= ro["iterations"] < 100
        assert np.abs(To - Tr).max() < 1e-5, c["name"]


def test_icp_tiny_targets(orc):
    """targets of 1, 2, 3 and 65 points are legal input: what the answer is"""
    rng = np.random.default_rng(12)
    for nt in (1, 2, 3, 65):
        It = nc.exactly(nc.slab(70 + nt, nt + 4, box=(4, 4, 1)), nt, nt)
        Is = It[rng.integers(0, nt, 300)] + rng.integers(-6, 7, (300, 3))
        src, tgt = nnr.lattice(Is), nnr.lattice(It)
        ref = nnr.icp_first_iteration(src, tgt, 2.0)
        To, ro = orc.icp_align(src, tgt, max_corr_dist=2.0, max_iterations=1)
        assert (ro["n_correspondences"], ro["state"], ro["iterations"]) == (ref["n"], ref["state"], ref["iterations"]) and ref["n"] == 300
        nnr.check_rigid(To, ref, src, tgt)
        if nt >= 3:
            assert np.abs(To - ref["T"]).max() <= nnr.t_tolerance(ref["T"]), nt
        fit = nnr.score(tgt, src, To)
        assert abs(ro["fitness"] - fit) <= nnr.sum_reorder_bound(300) * fit, nt


def test_rank_one_correlation_gives_a_proper_rotation(orc):
    """Regression: of a rank-1 correlation whose sums carry rounding noise, H v1 is that noise and not 0; normalised into U it gave an R
    that was not orthogonal (det 0.9976 on a two-point target).  The second singular value is now judged relative to the first."""
    for shape in ("two_points", "line"):
        src, tgt = nc.icp_rank_one_case(shape)
        ref = nnr.icp_first_iteration(src, tgt, 2.0)
        assert ref["n"] >= 200 and ref["singular"][1] < 1e-9 * ref["singular"][0], shape
        To, ro = orc.icp_align(src, tgt, max_corr_dist=2.0, max_iterations=1)
        assert (ro["n_correspondences"], ro["state"], ro["iterations"]) == (ref["n"], 1, 1)
        nnr.check_rigid(To, ref, src, tgt)
