"""The exact 1-NN search behind the fitness score and the loop-closure ICP (nn_search, fitness_wave, k_icp_accumulate), query by query.
-m gpu.

The lever (tests/nn_reference.py): on a dyadic lattice with an identity / lattice-translation / 90-degree pose every fp32 operation of
the score is exact and the fp64 sum is exact in any order, so the score must equal ``integer_sum * STEP^2 / n`` BIT FOR BIT and one
query with a wrong neighbour changes it.  Every case first asserts, from the reference alone, that it holds what its name says
(``query_class``: own_cell / block / far / outside / on_gate / beyond_gate, with a minimum count per class).  The cases are those of
tests/nn_cases.py, on which test_nn_reference.py has checked the C oracle against the same reference without a GPU.

ICP with max_iterations = 1 on lattice clouds: n_correspondences, state, iterations equal; final_T within 4 fp32 ulps of its largest
entry (test_nn_reference.py measures that ONE wrong correspondence moves T by at least 240 times that); fitness within n * 2^-52
relative (the bound on re-ordering a sum of n non-negative fp64 terms)."""
import numpy as np
import pytest

import nn_cases as nc
import nn_reference as nnr

pytestmark = pytest.mark.gpu

LATTICE = {c["name"]: c for c in nc.fitness_lattice_cases()}
I4 = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def reg():
    from rgc_slam_amd import registration
    return registration


def _vgicp(reg, res=1.0, k=20):
    v = reg.odometer_vgicp(0)
    v.setResolution(res)
    v.setCorrespondenceRandomness(k)
    return v


def _census(c, res):
    mv = nnr.lattice(nc.moved(c["Iq"], c["R"], c["t"]))
    cen = nnr.census(nnr.lattice(c["It"]), mv, res)
    for cls, least in c["need"].items():
        assert cen[cls] >= least, f"{c['name']} at cell size {res}: {cen}, needs {cls} >= {least}"


@pytest.mark.parametrize("name", sorted(LATTICE))
def test_score_on_lattice_bit_for_bit(reg, name):
    c = LATTICE[name]
    ref = nnr.lattice_score(c["It"], nc.moved(c["Iq"], c["R"], c["t"]))        # asserts its own preconditions
    for res in c["census_res"]:
        _census(c, res)
    tgt, src = nnr.lattice(c["It"]), nnr.lattice(c["Iq"])
    v = _vgicp(reg)
    for res in nc.RES:
        v.setResolution(res)
        v.setInputTarget(tgt)
        v.setInputSource(src)
        got = v.fitnessAt(c["T"])
        assert got == ref, f"{name} at cell size {res}: score {got!r}, reference {ref!r} (difference {got - ref:.3e} of {ref:.3e})"
    v.close()


def test_tail_case_has_the_cell_populations():
    c = LATTICE["cell_population_tails"]
    assert set(nnr.cell_histogram(nnr.lattice(c["It"]), 1.0).tolist()) == set(nc.TAIL_POPULATIONS)


@pytest.mark.parametrize("res", [0.3, 0.7, 1.9, 3.0])
def test_score_with_targets_an_ulp_off_the_walls(reg, res):
    """cell sizes that are not powers of two: target x on the fp32 nearest a wall (c + 0.5) * res and one ulp either side, queries
    straight across.  x is off the lattice, so the sum is compared within the re-ordering bound"""
    t, s = nc.wall_ulp_case(res)
    u = t[:, 0].astype(np.float64) / res - 0.5
    assert (np.abs(u - np.round(u)) * res <= 1.5 * np.spacing(np.abs(t[:, 0]))).all() and len(t) >= 2500
    ref = nnr.score(t, s)
    v = _vgicp(reg, res)
    v.setInputTarget(t)
    v.setInputSource(s)
    got = v.fitnessAt(I4)
    v.close()
    assert abs(got - ref) <= nnr.sum_reorder_bound(len(s)) * ref, f"cell size {res}: {got!r} vs {ref!r}"


@pytest.mark.parametrize("nt", nc.SMALL_NT)
def test_small_map_route_on_both_sides_of_its_limits(reg, nt):
    """targets of 32 767 / 32 768 / 32 769 points (the whole-wave scan's limit) and 511 .. 577 (its 8 x 64 and 64 tails), sources of which
    0 %, 2 %, 50 %, 100 % are `far` (waves with none, a few, more than four, 64 unsettled queries)"""
    v = _vgicp(reg, 1.0, k=2)
    for frac in nc.FAR_FRACTIONS:
        It, Iq = nc.small_map_case(nt, frac, 3000)
        assert len(It) == nt
        cen = nnr.census(nnr.lattice(It), nnr.lattice(Iq), 1.0)
        assert abs(cen["far"] - frac * 3000) <= 1 and cen["outside"] == 0, (nt, frac, cen)
        ref = nnr.lattice_score(It, Iq)
        v.setInputTarget(nnr.lattice(It))
        v.setInputSource(nnr.lattice(Iq))
        got = v.fitnessAt(I4)
        assert got == ref, f"nt = {nt}, {frac:.0%} far: score {got!r}, reference {ref!r}"
    v.close()


@pytest.mark.parametrize("nt", [512, 32768, 32769])
def test_small_map_route_deal_of_64k_queries(reg, nt):
    """ns = 64k and 64k +- 1: the `lane * W + w` deal of queries to waves"""
    v = _vgicp(reg, 1.0, k=2)
    for ns in (65535, 65536, 65537):
        for frac in (0.0, 0.02):
            It, Iq = nc.small_map_case(nt, frac, ns)
            occupied = set(map(tuple, nnr.cells(nnr.lattice(It), 1.0).tolist()))
            n_far = sum(tuple(c) not in occupied for c in nnr.cells(nnr.lattice(Iq), 1.0).tolist())
            assert abs(n_far - frac * ns) <= 1
            ref = nnr.lattice_score(It, Iq)
            v.setInputTarget(nnr.lattice(It))
            v.setInputSource(nnr.lattice(Iq))
            got = v.fitnessAt(I4)
            assert got == ref, f"nt = {nt}, ns = {ns}, {frac:.0%} far: score {got!r}, reference {ref!r}"
    v.close()


@pytest.mark.parametrize("n_map", [20000, 60000])
def test_the_three_score_kernels_agree(reg, monkeypatch, n_map):
    """k_lm_step's copy / k_fitness_lm (the score chained behind a solve) and k_fitness (fitnessAt): the same bits, under both LM drivers, on
    targets on both sides of 32 768 points; and within the re-ordering bound of the reference at that (non-lattice) pose"""
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(n_map, seed=synth.SEED + 3)
    assert (len(tgt) <= 32768) == (n_map == 20000)
    T_true = synth.se3(synth.rot_zyx(0.02, 0.002, -0.001), [0.12, 0.02, 0.001])
    src = synth.make_scan_n(world, T_true, 5000, seed=synth.SEED + 4)["xyz"]
    for impl in (None, "host"):
        if impl is None:
            monkeypatch.delenv("RGC_LM_IMPL", raising=False)
        else:
            monkeypatch.setenv("RGC_LM_IMPL", impl)
        v = reg.odometer_vgicp(0)
        v.setInputTarget(tgt)
        v.setInputSource(src)
        v.align(I4, want_output=False, want_fitness=True)
        chained, T = v.getFitnessScore(), v.getFinalTransformation()
        direct = v.fitnessAt(T)
        v.close()
        ref = nnr.score(tgt, src, T)
        assert chained == direct, f"RGC_LM_IMPL={impl}: chained {chained!r}, fitnessAt {direct!r}"
        assert abs(direct - ref) <= nnr.sum_reorder_bound(len(src)) * ref, f"RGC_LM_IMPL={impl}: {direct!r} vs {ref!r}"


def test_same_bits_from_a_lazy_a_reframed_and_a_borrowed_target(reg):
    c = LATTICE["sheet_and_poles"]
    tgt, src = nnr.lattice(c["It"]), nnr.lattice(c["Iq"])
    ref = nnr.lattice_score(c["It"], c["Iq"])
    v = _vgicp(reg)
    v.setLazyTarget(2)
    v.setInputTarget(tgt)
    v.setInputSource(src)
    assert v.fitnessAt(I4) == ref, "lazy target"
    v.setLazyTarget(0)
    # re-framed: the map re-expressed through an identity / a lattice translation (q * p + t in fp64, stored fp32: exact on the lattice)
    a = np.zeros((len(tgt), 4), np.float32)
    a[:, :3] = tgt
    d_map, d_body = v.device_alloc(a.nbytes), v.device_alloc(a.nbytes)
    v.upload(d_map, a)
    for t in ((0, 0, 0), (128, -64, 32)):
        v.setInputTargetReframed(d_map, len(tgt), 16, np.array([0.0, 0.0, 0.0, 1.0]), np.asarray(t, np.float64) * nnr.STEP, d_body)
        v.setInputSource(src)
        want = nnr.lattice_score(c["It"] + np.asarray(t), c["Iq"])
        got = v.fitnessAt(I4)
        assert got == want, f"re-framed by {t}: {got!r} vs {want!r}"
    # borrowed
    v.setInputTarget(tgt)
    w = _vgicp(reg)
    w.shareTargetFrom(v)
    w.setInputSource(src)
    assert w.fitnessAt(I4) == ref, "borrowed target"
    w.close()
    v.device_free(d_map); v.device_free(d_body)
    v.close()


# ---- ICP --------------------------------------------------------------------------------------------------------------------------------
class _OnDevice:
    """what IterativeClosestPoint accepts as a device cloud: (n, 4) float32 in memory of context `v`"""

    def __init__(self, v, xyz):
        a = np.zeros((len(xyz), 4), np.float32)
        a[:, :3] = xyz
        self._v, self._h, self.n, self.stride_bytes = v, v._h, len(xyz), 16
        self.ptr = v.device_alloc(a.nbytes)
        v.upload(self.ptr, a)
        v.synchronize()

    def __len__(self):
        return self.n

    def synchronize(self):
        self._v.synchronize()

    def free(self):
        self._v.device_free(self.ptr)


def _icp(gate, max_iterations):
    from rgc_slam_amd import loop_closure
    icp = loop_closure.IterativeClosestPoint(0)
    icp.setMaxCorrespondenceDistance(gate)
    icp.setMaximumIterations(max_iterations)
    icp.setTransformationEpsilon(1e-6)
    icp.setEuclideanFitnessEpsilon(1e-6)
    return icp


def _run_icp(reg, src, tgt, gate, max_iterations, device):
    icp = _icp(gate, max_iterations)
    if device:
        v = reg.odometer_vgicp(0)
        s, t = _OnDevice(v, src), _OnDevice(v, tgt)
        icp.setInputSource(s); icp.setInputTarget(t)
    else:
        icp.setInputSource(src); icp.setInputTarget(tgt)
    T = icp.align().copy()
    out = dict(T=T, n=int(icp._res.n_correspondences), state=int(icp._res.state), iterations=icp.nr_iterations, fitness=icp.getFitnessScore(),
               converged=icp.hasConverged())
    icp.close()
    if device:
        s.free(); t.free(); v.close()
    return out


def _check_first_iteration(name, got, ref, src, tgt, compare_T=True):
    assert (got["n"], got["state"], got["iterations"]) == (ref["n"], ref["state"], ref["iterations"]), \
        f"{name}: n / state / iterations {got['n'], got['state'], got['iterations']}, reference {ref['n'], ref['state'], ref['iterations']}"
    if ref["n"] >= 3:
        nnr.check_rigid(got["T"], ref, src, tgt)        # a proper rotation with the optimum's residual, also where Kabsch is not unique
    if compare_T:
        tol = nnr.t_tolerance(ref["T"])
        err = float(np.abs(got["T"].astype(np.float64) - ref["T"]).max())
        assert err <= tol, f"{name}: T differs by {err:.3e}, tolerance {tol:.3e}"
    fit = nnr.score(tgt, src, got["T"])
    assert abs(got["fitness"] - fit) <= nnr.sum_reorder_bound(len(src)) * fit, f"{name}: fitness {got['fitness']!r}, reference {fit!r}"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("gate", nc.ICP_GATES)
def test_icp_points_on_and_beyond_the_gate(reg, gate, device):
    Is, It = nc.icp_gate_case(gate)
    src, tgt = nnr.lattice(Is), nnr.lattice(It)
    cen = nnr.census(tgt, src, 1.0, gate)
    assert cen["beyond_gate"] >= 6 * len(It) and cen["on_gate"] >= (0 if gate == 0.3 else 6 * len(It)), cen
    _check_first_iteration(f"gate {gate}", _run_icp(reg, src, tgt, gate, 1, device), nnr.icp_first_iteration(src, tgt, gate), src, tgt)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_icp_exact_ties_take_the_smaller_original_index(reg, device):
    Is, It = nc.icp_tie_case()
    src, tgt = nnr.lattice(Is), nnr.lattice(It)
    i2, k2 = nnr.nearest_k(tgt, src, 2)
    tie = k2[:, 0] == k2[:, 1]
    order = np.lexsort((It[:, 0], It[:, 1], It[:, 2]))
    rank = np.empty(len(It), np.int64)
    rank[order] = np.arange(len(It))
    assert int(tie.sum()) >= 300 and int((rank[i2[tie, 0]] > rank[i2[tie, 1]]).sum()) >= 100     # index order is not cell order
    _check_first_iteration("ties", _run_icp(reg, src, tgt, 2.0, 1, device), nnr.icp_first_iteration(src, tgt, 2.0), src, tgt)


@pytest.mark.parametrize("n_kept", [0, 2, 3])
def test_icp_source_mostly_beyond_the_gate(reg, n_kept):
    Is, It, gate = nc.icp_few_case(n_kept)
    src, tgt = nnr.lattice(Is), nnr.lattice(It)
    ref = nnr.icp_first_iteration(src, tgt, gate)
    assert ref["n"] == n_kept and nnr.census(tgt, src, 1.0, gate)["beyond_gate"] >= 400
    got = _run_icp(reg, src, tgt, gate, 1, False)
    _check_first_iteration(f"{n_kept} kept", got, ref, src, tgt)
    if n_kept < 3:
        assert got["state"] == 5 and not got["converged"] and np.array_equal(got["T"], I4)


@pytest.mark.parametrize("shape", ["planar", "collinear"])
def test_icp_rank_deficient_correspondences(reg, shape):
    Is, It, gate = nc.icp_degenerate_case(shape)
    src, tgt = nnr.lattice(Is), nnr.lattice(It)
    ref = nnr.icp_first_iteration(src, tgt, gate)
    s = ref["singular"]
    assert s[2] < 1e-9 * s[0] and (shape == "planar") == (s[1] > 1e-3 * s[0])
    _check_first_iteration(shape, _run_icp(reg, src, tgt, gate, 1, False), ref, src, tgt, compare_T=(shape == "planar"))


@pytest.mark.parametrize("shape", ["two_points", "line"])
def test_icp_rank_one_correlation_off_the_lattice(reg, shape):
    """a target of two points / a kept set on one line with coordinates that are NOT exact: the sums carry rounding noise, the second
    singular value is that noise and not 0 (it used to be normalised into U: det R = 0.9976 on a two-point target)"""
    src, tgt = nc.icp_rank_one_case(shape)
    ref = nnr.icp_first_iteration(src, tgt, 2.0)
    assert ref["n"] >= 200 and ref["singular"][1] < 1e-9 * ref["singular"][0]
    _check_first_iteration(shape, _run_icp(reg, src, tgt, 2.0, 1, False), ref, src, tgt, compare_T=False)


@pytest.mark.parametrize("nt", [1, 2, 3, 65])
def test_icp_tiny_targets(reg, nt):
    """the grid route's rmax / whole-grid exits: targets of 1, 2, 3 and 65 points are legal input"""
    rng = np.random.default_rng(12)
    It = nc.exactly(nc.slab(70 + nt, nt + 4, box=(4, 4, 1)), nt, nt)
    Is = It[rng.integers(0, nt, 300)] + rng.integers(-6, 7, (300, 3))
    src, tgt = nnr.lattice(Is), nnr.lattice(It)
    ref = nnr.icp_first_iteration(src, tgt, 2.0)
    assert ref["n"] == 300
    _check_first_iteration(f"target of {nt}", _run_icp(reg, src, tgt, 2.0, 1, False), ref, src, tgt, compare_T=nt >= 3)


@pytest.mark.parametrize("case", nc.icp_loop_cases(), ids=lambda c: c["name"])
def test_icp_full_loop_on_other_generators(reg, case):
    Tr, rr = nnr.icp_align(case["src"], case["tgt"], gate=case["gate"])
    for device in (False, True):
        got = _run_icp(reg, case["src"], case["tgt"], case["gate"], 100, device)
        assert got["iterations"] == rr["iterations"], \
            f"{case['name']}: the two sides stop {abs(got['iterations'] - rr['iterations'])} iteration(s) apart ({got['iterations']} vs {rr['iterations']})"
        assert (got["state"], got["n"]) == (rr["state"], rr["n_correspondences"]) and got["converged"]
        assert np.abs(got["T"] - Tr).max() < 1e-5
        assert abs(got["fitness"] - rr["fitness"]) <= 1e-5 * rr["fitness"]
