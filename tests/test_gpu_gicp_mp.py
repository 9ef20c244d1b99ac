"""FastGICPMultiPoints (rgc_gicpmp_*) on the MI355X against the independent numpy reference tests/gicp_mp_reference.py, on the designed cases of
tests/gicp_mp_cases.py.

Rows (offsets, the members' indices and fp32 keys, none left out) and counts are compared for EQUALITY on every query of every case.  The merged values
are held to |difference| <= 2 count 2^-53 sum w |term| -- the weights are bit-equal by construction, only the order of an fp64 sum differs, and the bound
is that of two such sums.  cost / H / b are compared with the reference fed the product's own covariances from its getters, within the relative bound
tests/test_gpu_ndt.py and tests/test_gpu_gicp.py apply to the same (C_B + R C_A R^T)^-1 terms (1e-5: of the value for the cost, of the largest entry for H
and b); each test prints the product's difference next to what the reference differs from itself by (descending sums, adjugate against LU).  Whole solves:
iterations / converged / failed equal, the final pose within max(10 x the spread of two reference solves whose guesses differ by 1e-9, 4 fp32 ulps)."""
import numpy as np
import pytest

import gicp_mp_cases as mc
import gicp_mp_reference as mr
import ndt_reference as nr
import nn_reference as nn

pytestmark = pytest.mark.gpu

CENTER = mc.CENTER
REL = 1e-5          # tests/test_gpu_ndt.py, tests/test_gpu_gicp.py: the same (C_B + R C_A R^T)^-1 terms
U = 2.0 ** -53


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import gicp, registration
    return gicp, registration


def _product(mod, tgt, src, r, k=20, method=None):
    g = mod[0].FastGICPMultiPoints(0)
    g.setCorrespondenceRandomness(k)
    if method is not None:
        g.setRegularizationMethod(method)
    g.setNeighborSearchRadius(r)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    return g


def _reference(g, tgt, src, r):
    ref = mr.GICPMP(r)
    ref.set_target(tgt, g.getTargetCovariances())
    ref.set_source(src, g.getSourceCovariances())
    return ref


def _k_of(case):
    return case.get("k", 2 if min(len(case["tgt"]), len(case["src"])) < 20 else 20)


def _same_rows(g, rw):
    """the product's CSR rows equal the reference's on every query: offsets, and inside every row the members by ascending index with their keys"""
    off, idx, key = g.neighbors()
    assert np.array_equal(off.astype(np.int64), rw["off"]), np.flatnonzero(np.diff(off) != np.diff(rw["off"]))[:10]
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    o = np.lexsort((idx, row))
    bad = np.flatnonzero((idx[o] != rw["idx"]) | (key[o] != rw["key"]))
    assert bad.size == 0, (bad[:10], idx[o][bad[:10]], rw["idx"][bad[:10]], key[o][bad[:10]], rw["key"][bad[:10]])
    assert (g.num_correspondences, g.num_pairs) == (int((np.diff(rw["off"]) > 0).sum()), int(rw["off"][-1]))
    assert g.num_candidates >= g.num_pairs


def _same_merge(g, m):
    """count equal; sum_w, mean3, cov6 within 2 count 2^-53 sum w |term| of the reference; zeros behind a count of 0.  Returns the largest ratio to the bound."""
    cnt, sw, mean, cov = g.merged()
    assert np.array_equal(cnt, m["count"])
    none = cnt == 0
    assert not sw[none].any() and not mean[none].any() and not cov[none].any()
    c = 2.0 * cnt.astype(np.float64) * U
    worst = 0.0
    for got, want, mag in ((sw, m["sw"], m["sw"]), (mean, m["mean"], m["abs_mean"]), (cov, m["cov6"], m["abs_cov6"])):
        bound = (c if got.ndim == 1 else c[:, None]) * mag
        diff = np.abs(got - want)
        assert (diff <= bound).all(), (np.argwhere(diff > bound)[:5], diff.max())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, diff / bound, 0.0), initial=0.0)))
    return worst


def _rel(y, H, b, yr, Hr, br):
    return (abs(y - yr) / max(abs(yr), 1e-300), np.abs(H - Hr).max() / max(np.abs(Hr).max(), 1e-300), np.abs(b - br).max() / max(np.abs(br).max(), 1e-300))


def _check_terms(g, ref, T, label, rows=None):
    y, H, b = g.linearize(T)
    if rows is None:
        ya, Ha, ba = ref.linearize(T)
        yr, Hr, br = ref.linearize(T, descending=True, inverse=mr.adjugate_inverse)
    else:                                                       # the rows of this pose are known: only the merge and the terms are computed
        out = []
        for desc, inv in ((False, np.linalg.inv), (True, mr.adjugate_inverse)):
            m = ref.merge(T, desc, rows=rows)
            _, l, J, _ = ref.loss_rows(T, m, inv)
            out.append((float(mr.ordered_sum(np.einsum("ni,ni->n", l, l), desc)), mr.ordered_sum(np.einsum("nia,nib->nab", J, J), desc),
                        mr.ordered_sum(np.einsum("nia,ni->na", J, l), desc)))
        (ya, Ha, ba), (yr, Hr, br) = out
    spread = max(_rel(yr, Hr, br, ya, Ha, ba))
    errs = _rel(y, H, b, ya, Ha, ba)
    print("%s: product - reference %.3g relative, reference - itself (descending sums, adjugate) %.3g; bound %.1g (16 x spread = %.3g)"
          % (label, max(errs), spread, REL, 16 * spread))
    assert max(errs) <= REL, (label, errs)
    assert np.array_equal(H, H.T)
    y2, H2, b2 = g.linearize(T)
    assert y2 == y and np.array_equal(H2, H) and np.array_equal(b2, b)                  # the same bits from run to run ...
    assert g.linearize(T, want_H=False)[0] == y                                          # ... and without H
    return max(errs), spread


# ---- every case: rows, counts, merged values, terms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.all_cases(), ids=lambda c: c["name"])
def test_case(mod, case):
    tgt, src, r = case["tgt"], case["src"], case["r"]
    g = _product(mod, tgt, src, r, k=_k_of(case))
    ref = _reference(g, tgt, src, r)
    for p, T in enumerate(case["poses"]):
        rw = mc.rows_of(case["name"], p)
        g.linearize(T, want_H=False)
        _same_rows(g, rw)
        m = ref.merge(T, rows=rw)
        ratio = _same_merge(g, m)
        print("%s pose %d: %d queries, %d with a neighbour, %d neighbours (longest row %d); merged values at most %.3g of their bound"
              % (case["name"], p, len(src), int((m["count"] > 0).sum()), int(m["count"].sum()), int(m["count"].max()), ratio))
        if (m["count"] > 0).any():
            _check_terms(g, ref, T, "%s pose %d" % (case["name"], p), rows=rw)
        else:
            y, H, b = g.linearize(T)
            assert y == 0.0 and not H.any() and not b.any()
    g.close()


def test_one_point_target_is_refused(mod):
    """k >= 2 and a cloud of at least k points: the context's rule for every cloud, as for FastGICP"""
    g = mod[0].FastGICPMultiPoints(0)
    g.setCorrespondenceRandomness(2)
    with pytest.raises(mod[0].RgcError):
        g.setInputTarget(mc.scene_data()["tgt"][:1])
    g.close()


# ---- covariance routes ---------------------------------------------------------------------------------------------------------------------------
def _small():
    d = mc.scene_data()
    return d["tgt"][::2], d["src"][:3000], d["T"]


@pytest.mark.parametrize("general_src,general_tgt", [(False, False), (False, True), (True, False), (True, True)])
def test_terms_on_the_four_covariance_route_pairs(mod, general_src, general_tgt):
    """tuned (PLANE: a unit normal per point) and general (MIN_EIG: six doubles per point) covariances for source and target; a mixed pair is a borrowed
    target, whose route is its owner's"""
    tgt, src, T = _small()
    reg = mod[1].FastVGICP
    owner = None
    if general_src == general_tgt:
        g = _product(mod, tgt, src, 0.5, method=reg.REG_MIN_EIG if general_src else None)
    else:
        owner = mod[1].FastVGICP(0)
        if general_tgt:
            owner.setRegularizationMethod(reg.REG_MIN_EIG)
        owner.setInputTarget(tgt)
        g = mod[0].FastGICPMultiPoints(0)
        if general_src:
            g.setRegularizationMethod(reg.REG_MIN_EIG)
        g.setNeighborSearchRadius(0.5)
        g.shareTargetFrom(owner)
        g.setInputSource(src)
    ref = mr.GICPMP(0.5)
    ref.set_target(tgt, (owner or g).getTargetCovariances())
    ref.set_source(src, g.getSourceCovariances())
    plane = lambda C: np.abs(np.linalg.eigvalsh(C) - np.array([1e-3, 1.0, 1.0])).max() < 1e-9
    assert plane(ref.cov_s[0]) != general_src and plane(ref.cov_t[0]) != general_tgt
    for P in (T, np.eye(4)):
        rw = ref.rows(P)
        g.linearize(P, want_H=False)
        _same_rows(g, rw)
        _same_merge(g, ref.merge(P, rows=rw))
        _check_terms(g, ref, P, "source %s, target %s" % ("general" if general_src else "tuned", "general" if general_tgt else "tuned"), rows=rw)
    g.close()
    if owner is not None:
        owner.close()


@pytest.mark.parametrize("n", [2, 63, 257, 16500])
def test_terms_block_sum_and_fold_shapes(mod, n):
    """the term kernel's block sums and the fold at source sizes of a partial wave (63), a second workgroup of one lane (257) and more than 64 partial
    rows (16500: the fold's second stride).  One lane alone cannot be had: a cloud needs at least k = 2 points (test_one_point_target_is_refused), so
    the smallest source is 2 points.  The same reference and bound as every other term test here."""
    d = mc.scene_data()
    tgt, T = d["tgt"][:4000], d["T"]
    rng = np.random.default_rng(4200 + n)
    Ti = np.linalg.inv(T)                                       # noisy copies of target points seen from T: every ball holds at least its own point
    src = (tgt[rng.choice(len(tgt), n, replace=n > len(tgt))].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    g = _product(mod, tgt, src, 0.5, k=2 if n < 20 else 20)
    ref = _reference(g, tgt, src, 0.5)
    _check_terms(g, ref, T, "source of %d" % n)
    assert g.num_correspondences == n
    g.close()


def test_terms_with_user_set_covariances(mod):
    tgt, src, T = _small()
    donor = _product(mod, tgt, src, 0.5, k=8)
    ct, cs = donor.getTargetCovariances(), donor.getSourceCovariances()
    donor.close()
    g = _product(mod, tgt, src, 0.5)
    own = g.linearize(T)[0]
    g.setTargetCovariances(ct)
    g.setSourceCovariances(cs)
    ref = _reference(g, tgt, src, 0.5)
    assert np.abs(ref.cov_t - ct).max() <= 2e-9 and np.abs(ref.cov_s - cs).max() <= 2e-9
    _check_terms(g, ref, T, "user-set covariances")
    assert g.linearize(T)[0] != own
    g.close()


# ---- the same bits on every route ------------------------------------------------------------------------------------------------------------------
def _everything(g, T):
    y, H, b = g.linearize(T)
    return (np.float64(y), H, b) + g.merged() + g.neighbors()


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_routes_give_identical_bits(mod):
    tgt, src, T = _small()
    plain = _product(mod, tgt, src, 0.5)
    base = _everything(plain, T)
    assert _same_bits(base, _everything(plain, T)), "two runs"
    d = mod[0].FastGICPMultiPoints(0)                           # device pointers
    d.setNeighborSearchRadius(0.5)
    t4, s4 = np.zeros((len(tgt), 4), np.float32), np.zeros((len(src), 4), np.float32)
    t4[:, :3], s4[:, :3] = tgt, src
    pt, ps = d.device_alloc(t4.nbytes), d.device_alloc(s4.nbytes)
    d.upload(pt, t4); d.upload(ps, s4)
    d.setInputTargetDevice(pt, len(tgt), 16); d.setInputSourceDevice(ps, len(src), 16)
    assert _same_bits(base, _everything(d, T)), "device pointers"
    lz = mod[0].FastGICPMultiPoints(0)                          # lazy target: completed first
    lz.setNeighborSearchRadius(0.5)
    lz.setLazyTarget(2)
    lz.setInputTarget(tgt); lz.setInputSource(src)
    assert _same_bits(base, _everything(lz, T)), "lazy target"
    bo = mod[0].FastGICPMultiPoints(0)                          # borrowed target
    bo.setNeighborSearchRadius(0.5)
    bo.shareTargetFrom(plain)
    bo.setInputSource(src)
    assert _same_bits(base, _everything(bo, T)), "borrowed target"
    d.device_free(pt); d.device_free(ps)
    for x in (bo, plain, d, lz):
        x.close()


# ---- whole solves --------------------------------------------------------------------------------------------------------------------------------------
def _pose_error(X, T):
    d = np.asarray(X, np.float64) @ np.linalg.inv(T)
    return float(np.linalg.norm(d[:3, 3] - (np.eye(3) - d[:3, :3]) @ np.array(CENTER))), float(np.abs(d[:3, :3] - np.eye(3)).max())


@pytest.mark.parametrize("r", [0.25, 0.5])
def test_whole_solves(mod, r):
    d = mc.scene_data()
    tgt, src, T = d["tgt"][::3], d["src"][:2000], d["T"]
    g = _product(mod, tgt, src, r)
    ref = _reference(g, tgt, src, r)
    rng = np.random.default_rng(3)
    for guess in (np.eye(4), nr.random_pose(rng, max_t=0.05, max_deg=0.5, about=CENTER) @ T):
        g32 = guess.astype(np.float32)
        X, iters, conv, failed, Hfin = ref.align(g32)
        X2 = ref.align(g32, perturb=1e-9)[0]
        spread = float(np.abs(X - X2).max())
        tol = max(10 * spread, nn.t_tolerance(X))
        g.align(g32, want_output=False, want_fitness=True)
        got = g.getFinalTransformation()
        diff = float(np.abs(got.astype(np.float64) - X).max())
        et, _ = _pose_error(got, T)
        rt, _ = _pose_error(X, T)
        print("r %g: %d iterations (reference %d), converged %d/%d, failed %d/%d; |T - T_ref| = %.3g, tolerance %.3g (reference spread under a 1e-9 guess change %.3g); "
              "pose error %.4f m (reference %.4f m)" % (r, g.nr_iterations, iters, g.hasConverged(), conv, g.lm_failed, failed, diff, tol, spread, et, rt))
        assert (g.nr_iterations, g.hasConverged(), g.lm_failed) == (iters, conv, failed)
        assert conv and not failed
        assert diff <= tol
        assert np.abs(g.getFinalHessian() - Hfin).max() <= REL * np.abs(Hfin).max()
        assert g.getFitnessScore() == pytest.approx(nn.score(tgt, src, got), rel=nn.sum_reorder_bound(len(src)))
    g.setMaximumIterations(2)                                   # the limit ends a solve that has not converged: no flag raised
    X, iters, conv, failed, _ = ref.align(np.eye(4, dtype=np.float32), max_iterations=2)
    g.align(np.eye(4), want_output=False)
    assert (g.nr_iterations, g.hasConverged(), g.lm_failed) == (iters, conv, failed) == (2, False, False)
    g.close()


def test_a_moved_scan_is_recovered(mod):
    """SURVEY section 4's property: T . cloud registered against cloud for random small SE(3) (<= 0.3 m, <= 3 degrees) with sensor noise (5 mm) -> the
    recovered pose within 1e-3 (metres at the scene's centre, and entries of the rotation)"""
    rng = np.random.default_rng(77)
    cloud = nr.scene(rng, 8000)
    g = mod[0].FastGICPMultiPoints(0)
    g.setInputTarget(cloud)
    for _ in range(3):
        T = nr.random_pose(rng, about=CENTER)
        Ti = np.linalg.inv(T)
        src = (cloud.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.005, (len(cloud), 3))).astype(np.float32)
        g.setInputSource(src)
        g.align(np.eye(4), want_output=False)
        et, er = _pose_error(g.getFinalTransformation(), T)
        print("%d iterations, converged %d: pose error %.2e m, %.2e in the rotation" % (g.nr_iterations, g.hasConverged(), et, er))
        assert g.hasConverged() and not g.lm_failed
        assert et <= 1e-3 and er <= 1e-3
    g.close()


def test_a_source_with_no_neighbour_anywhere_fails_at_the_guess(mod):
    tgt, src, T = _small()
    g = _product(mod, tgt, src, 0.5)
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = [500.0, 500.0, 50.0]
    y, H, b = g.linearize(far.astype(np.float64))
    assert y == 0.0 and not H.any() and not b.any() and (g.num_correspondences, g.num_pairs) == (0, 0)
    off, idx, key = g.neighbors()
    assert not off.any() and len(idx) == 0 and not g.merged()[0].any()
    g.align(far, want_output=False)
    assert (g.nr_iterations, g.hasConverged(), g.lm_failed) == (1, False, True)
    assert np.array_equal(g.getFinalTransformation(), far)
    g.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------------------------
def test_kept_results_drop_and_bad_arguments_are_refused(mod):
    import ctypes as C
    tgt, src, T = _small()
    g = _product(mod, tgt, src, 0.5)
    reads = (lambda: g.num_correspondences, lambda: g.merged(), lambda: g.neighbors(cap=10 ** 6))
    for refused in reads:
        with pytest.raises(mod[0].RgcError):
            refused()                                           # no linearisation yet
    drops = [lambda: g.setInputSource(src), lambda: g.setInputTarget(tgt), lambda: g.setSourceCovariances(g.getSourceCovariances()),
             lambda: g.setTargetCovariances(g.getTargetCovariances()), lambda: g.setCorrespondenceRandomness(12), lambda: (g.clearSource(), g.setInputSource(src)),
             lambda: g.setNeighborSearchRadius(0.5), lambda: g.setRotationEpsilon(1e-5)]
    for drop in drops:
        g.linearize(T, want_H=False)
        assert g.num_pairs > 0
        drop()
        for refused in reads:
            with pytest.raises(mod[0].RgcError):
                refused()
    g.linearize(T, want_H=False)
    total = g.num_pairs
    off, idx, key = np.full(len(src) + 1, -7, np.int32), np.full(total, -7, np.int32), np.zeros(total, np.float32)
    nt = C.c_longlong(0)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    rc = g._L.rgc_gicpmp_get_neighbors(g._h, off.ctypes.data_as(ip), idx.ctypes.data_as(ip), key.ctypes.data_as(fp), total - 1, C.byref(nt))
    assert rc == -1 and nt.value == total and (off == -7).all() and (idx == -7).all()   # a too-small cap: the total is told, no row is written
    assert g._L.rgc_gicpmp_get_neighbors(g._h, off.ctypes.data_as(ip), idx.ctypes.data_as(ip), key.ctypes.data_as(fp), total, C.byref(nt)) == 0
    assert off[0] == 0 and off[-1] == total and (idx >= 0).all()
    for bad in (0.0, -1.0, np.nan, np.inf, 1e30):               # (1e30: float(r r) is not finite)
        with pytest.raises(mod[0].RgcError):
            g.setNeighborSearchRadius(bad)
    assert g.getNeighborSearchRadius() == 0.5
    for setter, bad in ((g.setMaximumIterations, 0), (g.setRotationEpsilon, 0.0), (g.setTransformationEpsilon, -1.0), (g.setRotationEpsilon, np.nan)):
        with pytest.raises(mod[0].RgcError):
            setter(bad)
    nanT = np.eye(4)
    nanT[0, 3] = np.nan
    with pytest.raises(mod[0].RgcError):
        g.linearize(nanT)
    g.clearSource()
    for refused in (lambda: g.linearize(T), lambda: g.align(np.eye(4), want_output=False)):
        with pytest.raises(mod[0].RgcError) as e:
            refused()
        assert e.value.status == -1
    g.close()


def test_refused_with_a_solve_in_flight(mod):
    tgt, src, T = _small()
    g = _product(mod, tgt, src, 0.5)
    guess = np.eye(4, dtype=np.float32)
    g.linearize(T, want_H=False)
    g.align_begin(guess)
    for refused in (lambda: g.linearize(T), lambda: g.align(guess, want_output=False), lambda: g.num_correspondences, lambda: g.merged(), lambda: g.neighbors(cap=10 ** 6),
                    lambda: g.setNeighborSearchRadius(0.3)):
        with pytest.raises(mod[0].RgcError):
            refused()
    g.align_end()
    g.linearize(T, want_H=False)
    g.close()


def test_cpp_mirror_runs(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "rgc-slam_amd")
    exe = tmp_path / "test_gicp_mp"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(root, "tests", "cpp", "test_gicp_mp.cpp"), "-o", str(exe),
                           "-L", pkg, "-lrgc_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
