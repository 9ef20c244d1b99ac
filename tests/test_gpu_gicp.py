"""FastGICP (rgc_gicp_*) on the MI355X against the independent numpy reference tests/gicp_reference.py.

Correspondences (index and fp32 key per source point, none left out) are compared for EQUALITY.  cost / H / b are compared with the reference fed the
product's own covariances from its getters, within the relative bound tests/test_gpu_ndt.py applies to the same D2D expression (1e-5: of the value for
the cost, of the largest entry for H and b); each test also prints what the reference differs from itself by when it sums in descending order and inverts
by the adjugate, and the product's own difference.  Whole solves: iterations / converged / lm_failed equal, the final pose within max(10 x the spread of
two reference solves whose guesses differ by 1e-9, 4 fp32 ulps of its largest entry).

One case of the issue cannot be constructed: a target of ONE point.  The context's clouds need at least k points and k >= 2 (rgc_set_params, RGC_ERR_TOO_FEW_POINTS;
the reference computes a covariance from the k nearest neighbours of every point): test_tiny_targets asserts that refusal for 1 point and compares 2, 3 and 65."""
import numpy as np
import pytest

import gicp_reference as gr
import ndt_reference as nr
import nn_cases
import nn_reference as nn

pytestmark = pytest.mark.gpu

CENTER = (100.0, -60.0, 2.0)
REL = 1e-5          # tests/test_gpu_ndt.py, test_linearize_and_compute_error: the same (C_B + R C_A R^T)^-1 terms


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import gicp, registration
    return gicp, registration


@pytest.fixture(scope="module")
def data():
    """a 24 k map, an 8 k scan of it seen from a pose within 0.3 m / 3 deg (1 cm of noise), that pose and three more"""
    rng = np.random.default_rng(9101)
    tgt = nr.scene(rng, 24000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (nr.scene(rng, 8000).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (8000, 3))).astype(np.float32)
    return dict(tgt=tgt, src=src, T=T, poses=[np.eye(4), T] + [nr.random_pose(rng, about=CENTER) for _ in range(3)])


def _product(mod, tgt, src, k=20, method=None, d_max=None):
    g = mod[0].FastGICP(0)
    g.setCorrespondenceRandomness(k)
    if method is not None:
        g.setRegularizationMethod(method)
    if d_max is not None:
        g.setMaxCorrespondenceDistance(d_max)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    return g


def _reference(g, tgt, src, d_max=gr.FLT_MAX):
    ref = gr.GICP(d_max)
    ref.set_target(tgt, g.getTargetCovariances())
    ref.set_source(src, g.getSourceCovariances())
    return ref


def _same_pairs(g, ref, T):
    """the product's pair list at T equals the reference's on every query; returns (idx, key)"""
    idx, key = g.correspondences()
    ridx, rkey = ref.correspondences(T)
    assert idx.shape == ridx.shape == key.shape
    bad = np.flatnonzero((idx != ridx) | (key != rkey))
    assert bad.size == 0, (bad[:10], idx[bad[:10]], ridx[bad[:10]], key[bad[:10]], rkey[bad[:10]])
    assert g.num_correspondences == int((ridx >= 0).sum())
    return ridx, rkey


def _rel(y, H, b, yr, Hr, br):
    return (abs(y - yr) / max(abs(yr), 1e-300), np.abs(H - Hr).max() / np.abs(Hr).max(), np.abs(b - br).max() / max(np.abs(br).max(), 1e-300))


def _check_terms(g, ref, poses, label):
    """cost, H, b at every pose and the frozen cost at three poses away from it, against the reference; prints the product's difference next to the
    reference's difference from itself (descending sums, adjugate inverses)"""
    worst = spread = 0.0
    for T in poses:
        y, H, b = g.linearize(T)
        yr, Hr, br = ref.linearize(T, descending=True, inverse=gr.adjugate_inverse)
        ya, Ha, ba = ref.linearize(T)                          # (last: the frozen list compute_error below uses is the plain one)
        _same_pairs(g, ref, T)
        assert ref.num_kept() > 0
        spread = max(spread, *_rel(yr, Hr, br, ya, Ha, ba))
        errs = _rel(y, H, b, ya, Ha, ba)
        worst = max(worst, *errs)
        assert max(errs) <= REL, (label, errs)
        assert np.array_equal(H, H.T)
        assert g.linearize(T, want_H=False)[0] == y            # the same bits from run to run, with and without H
        assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
        for d in ([0.002, -0.001, 0.003, 0.01, -0.02, 0.015], [-0.004, 0.002, 0.001, -0.03, 0.01, 0.02], [0.0, 0.0, 0.01, 0.05, 0.05, -0.05]):
            T3 = nr.increment(np.array(d), T)[0]
            e, er = g.compute_error(T3), ref.compute_error(T3)
            assert abs(e - er) <= REL * abs(er), (label, e, er)
            worst = max(worst, abs(e - er) / abs(er))
    print("%s: %d pairs; product - reference %.3g relative, reference - itself (descending sum, adjugate) %.3g; bound %.1g (16 x spread = %.3g)"
          % (label, ref.num_kept(), worst, spread, REL, 16 * spread))
    return worst, spread


# ---- correspondences ------------------------------------------------------------------------------------------------------------------
def test_scene_correspondences_are_exact(mod, data):
    g = _product(mod, data["tgt"], data["src"])
    ref = _reference(g, data["tgt"], data["src"])
    for T in data["poses"]:
        g.linearize(T, want_H=False)
        idx, _ = _same_pairs(g, ref, T)
        assert (idx >= 0).all()                                 # the default maximum distance rejects nothing
    g.setMaxCorrespondenceDistance(0.05)
    ref.d_max = 0.05
    g.linearize(data["T"], want_H=False)
    idx, _ = _same_pairs(g, ref, data["T"])
    assert 500 <= (idx >= 0).sum() <= len(idx) - 500
    assert g.getMaxCorrespondenceDistance() == 0.05
    g.close()


@pytest.mark.parametrize("case", [c for c in nn_cases.fitness_lattice_cases()
                                  if c["name"] in ("dense_slab", "dense_slab_rz90_shift", "sheet_and_poles", "points_on_walls", "cell_population_tails", "cut_map_far_source")],
                         ids=lambda c: c["name"])
def test_lattice_correspondences_are_exact(mod, case):
    """dyadic lattice clouds: every key is an exact integer multiple of 2^-12, exact ties are common and the gate (3 lattice units: keys of exactly
    9 units^2 lie ON it and are rejected, 8 units^2 one step inside it are kept) is hit exactly.  How many ties and gate points a case holds is counted
    by the reference alone."""
    tgt, src, T = nn.lattice(case["It"]), nn.lattice(case["Iq"]), case["T"].astype(np.float64)
    gate = 3 * nn.STEP
    g = _product(mod, tgt, src, k=5, d_max=gate)
    ref = gr.GICP(gate)
    ref.set_target(tgt, np.broadcast_to(np.eye(3), (len(tgt), 3, 3)))
    ref.set_source(src, np.broadcast_to(np.eye(3), (len(src), 3, 3)))
    g.linearize(T, want_H=False)
    idx, key = _same_pairs(g, ref, T)
    q = nn.transform_f32(src, T.astype(np.float32))
    _, k2 = nn.nearest_k(tgt, q, 2)
    ties, on_gate, inside = int((k2[:, 0] == k2[:, 1]).sum()), int((key == np.float32(gate * gate)).sum()), int((key == np.float32(8 * nn.STEP ** 2)).sum())
    print("%s: %d queries, %d exact ties, %d on the gate, %d one step inside it, %d kept" % (case["name"], len(src), ties, on_gate, inside, (idx >= 0).sum()))
    # minima from the reference alone (measured with tests/nn_reference.py on these cases: dense_slab 327 queries on the gate, 148 one step inside it,
    # 1145 kept of 8000; sheet_and_poles 817 exact ties; points_on_walls 127)
    if case["name"] == "dense_slab":
        assert on_gate >= 300 and inside >= 100 and 1000 <= (idx >= 0).sum() <= len(idx) - 1000
    if case["name"] == "sheet_and_poles":
        assert ties >= 800
    if case["name"] == "points_on_walls":
        assert ties >= 100
    assert not (idx[key >= np.float32(gate * gate)] >= 0).any() and (idx[key < np.float32(gate * gate)] >= 0).all()
    g.setMaxCorrespondenceDistance(gr.FLT_MAX)
    ref.d_max = gr.FLT_MAX
    g.linearize(T, want_H=False)
    idx, _ = _same_pairs(g, ref, T)
    assert (idx >= 0).all()
    g.close()


def test_tiny_targets(mod, data):
    src = data["src"][:500]
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 65):
        tgt = data["tgt"][rng.choice(len(data["tgt"]), n, replace=False)]
        g = mod[0].FastGICP(0)
        g.setCorrespondenceRandomness(2)
        if n == 1:                                              # k >= 2 and a cloud of at least k points: the context's rule for every cloud
            with pytest.raises(mod[0].RgcError):
                g.setInputTarget(tgt)
            g.close()
            continue
        g.setInputTarget(tgt)
        g.setInputSource(src)
        ref = _reference(g, tgt, src)
        for T in (np.eye(4), data["T"]):
            g.linearize(T, want_H=False)
            idx, _ = _same_pairs(g, ref, T)
            assert (idx >= 0).all() and len(np.unique(idx)) <= n
        g.close()


# ---- terms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 10, 20, 32])
def test_terms_plane_tuned_route(mod, data, k):
    g = _product(mod, data["tgt"], data["src"], k=k)
    ref = _reference(g, data["tgt"], data["src"])
    _check_terms(g, ref, [data["T"], np.eye(4)], "PLANE k=%d" % k)
    g.close()


@pytest.mark.parametrize("name", ["REG_MIN_EIG", "REG_NORMALIZED_MIN_EIG", "REG_FROBENIUS"])
@pytest.mark.parametrize("k", [10, 20])
def test_terms_general_route(mod, data, name, k):
    g = _product(mod, data["tgt"][:12000], data["src"][:3000], k=k, method=getattr(mod[1].FastVGICP, name))
    ref = _reference(g, data["tgt"][:12000], data["src"][:3000])
    _check_terms(g, ref, [data["T"], np.eye(4)], "%s k=%d" % (name, k))
    g.close()


@pytest.mark.parametrize("n", [2, 63, 257, 16500])
def test_terms_block_sum_and_fold_shapes(mod, data, n):
    """the term kernel's block sums and the fold at source sizes of a partial wave (63), a second workgroup of one lane (257) and more than 64 partial
    rows (16500: the fold's second stride).  One lane alone cannot be had: a cloud needs at least k = 2 points (test_tiny_targets), so the smallest
    source is 2 points.  The same reference and bound as every other term test here."""
    rng = np.random.default_rng(4100 + n)
    Ti = np.linalg.inv(data["T"])
    src = (nr.scene(rng, n).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    tgt = data["tgt"][:6000]
    g = _product(mod, tgt, src, k=2 if n < 20 else 20)
    ref = _reference(g, tgt, src)
    _check_terms(g, ref, [data["T"]], "source of %d" % n)
    assert g.num_correspondences == n
    g.close()


def test_terms_without_regularisation_on_a_volumetric_cloud(mod):
    """REG_NONE keeps the raw kNN covariance: only a cloud that fills a volume (uniform in a box, noisy) has covariances that can be inverted"""
    rng = np.random.default_rng(77)
    tgt = (rng.uniform(-4, 4, (9000, 3)) + np.array(CENTER)).astype(np.float32)
    T = nr.random_pose(rng, max_t=0.1, max_deg=1.0, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (tgt[::3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.02, (3000, 3))).astype(np.float32)
    g = _product(mod, tgt, src, k=20, method=mod[1].FastVGICP.REG_NONE)
    ref = _reference(g, tgt, src)
    _check_terms(g, ref, [T, np.eye(4)], "NONE k=20")
    g.close()


def test_terms_with_user_set_covariances(mod, data):
    donor = _product(mod, data["tgt"], data["src"], k=8)
    ct, cs = donor.getTargetCovariances(), donor.getSourceCovariances()
    donor.close()
    g = _product(mod, data["tgt"], data["src"], k=20)
    own = g.linearize(data["T"])[0]
    g.setTargetCovariances(ct)
    with pytest.raises(mod[0].RgcError):
        g.compute_error(data["T"])                              # new covariances: the frozen list is gone
    g.setSourceCovariances(cs)
    ref = _reference(g, data["tgt"], data["src"])
    # (a matrix is accepted within 1e-9 of the PLANE form and kept as its unit normal: the getter may differ from what was set by that much and its own rounding)
    assert np.abs(ref.cov_t - ct).max() <= 2e-9 and np.abs(ref.cov_s - cs).max() <= 2e-9
    _check_terms(g, ref, [data["T"], np.eye(4)], "user-set covariances")
    assert g.linearize(data["T"])[0] != own
    g.close()


# ---- the frozen list's life -------------------------------------------------------------------------------------------------------------
def test_compute_error_is_refused_after_what_drops_the_list(mod, data):
    tgt, src, T = data["tgt"], data["src"], data["T"]
    g = _product(mod, tgt, src)
    with pytest.raises(mod[0].RgcError):
        g.compute_error(T)                                      # no linearisation yet
    with pytest.raises(mod[0].RgcError):
        g.num_correspondences
    drops = [lambda: g.setInputSource(src), lambda: g.setInputTarget(tgt), lambda: g.setSourceCovariances(g.getSourceCovariances()),
             lambda: g.setTargetCovariances(g.getTargetCovariances()), lambda: (g.swapSourceAndTarget(), g.swapSourceAndTarget()),
             lambda: g.setCorrespondenceRandomness(12), lambda: g.setResolution(2.0), lambda: (g.clearSource(), g.setInputSource(src)),
             lambda: (g.clearTarget(), g.setInputTarget(tgt))]
    for drop in drops:
        y = g.linearize(T, want_H=False)[0]
        assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
        drop()
        for refused in (lambda: g.compute_error(T), lambda: g.num_correspondences, lambda: g.correspondences()):
            with pytest.raises(mod[0].RgcError):
                refused()
    y = g.linearize(T, want_H=False)[0]
    g.setMaxCorrespondenceDistance(0.5)                         # a new gate leaves the list in force until the next linearisation
    assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
    g.clearSource()
    for refused in (lambda: g.linearize(T), lambda: g.align(np.eye(4), want_output=False)):
        with pytest.raises(mod[0].RgcError) as e:
            refused()
        assert e.value.status == -1
    g.setInputSource(src)
    bad = np.eye(4)
    bad[0, 3] = np.nan
    with pytest.raises(mod[0].RgcError):
        g.linearize(bad)
    with pytest.raises(mod[0].RgcError):
        g.setMaxCorrespondenceDistance(-1.0)
    g.close()


def _everything(g, T):
    y, H, b = g.linearize(T)
    idx, key = g.correspondences()
    T3 = nr.increment(np.array([0.002, -0.001, 0.003, 0.01, -0.02, 0.015]), T)[0]
    return (np.float64(y), H, b, idx, key, np.float64(g.compute_error(T3)))


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_routes_give_identical_bits(mod, data):
    from rgc_slam_amd import local_map
    tgt, src, T = data["tgt"], data["src"], data["T"]
    plain = _product(mod, tgt, src)
    base = _everything(plain, T)
    assert _same_bits(base, _everything(plain, T)), "two runs"
    # device pointers
    d = mod[0].FastGICP(0)
    t4, s4 = np.zeros((len(tgt), 4), np.float32), np.zeros((len(src), 4), np.float32)
    t4[:, :3], s4[:, :3] = tgt, src
    pt, ps = d.device_alloc(t4.nbytes), d.device_alloc(s4.nbytes)
    d.upload(pt, t4); d.upload(ps, s4)
    d.setInputTargetDevice(pt, len(tgt), 16); d.setInputSourceDevice(ps, len(src), 16)
    assert _same_bits(base, _everything(d, T)), "device pointers"
    # lazy target
    lz = mod[0].FastGICP(0)
    lz.setLazyTarget(2)
    lz.setInputTarget(tgt); lz.setInputSource(src)
    assert _same_bits(base, _everything(lz, T)), "lazy target"
    # borrowed target
    bo = mod[0].FastGICP(0)
    bo.shareTargetFrom(plain)
    bo.setInputSource(src)
    assert _same_bits(base, _everything(bo, T)), "borrowed target"
    # re-framed target: compared with a plain target of the re-framed points
    body_ptr = d.device_alloc(t4.nbytes)
    q, t = np.array([0.0, 0.0, np.sin(0.05), np.cos(0.05)]), np.array([0.3, -0.2, 0.01])
    d.setInputTargetReframed(pt, len(tgt), 16, q, t, body_ptr)
    body = d.download(body_ptr, (len(tgt), 4))[:, :3].copy()
    rf = _everything(d, T)
    p2 = _product(mod, body, src)
    assert _same_bits(_everything(p2, T), rf), "re-framed target"
    d.setInputTargetReframed(pt, len(tgt), 16, q, t, body_ptr)   # again: neighbour lists re-used
    assert _same_bits(rf, _everything(d, T)), "re-framed target, second frame"
    # map-bound target: compared with a plain target of the committed cloud
    mb = mod[0].FastGICP(0)
    lm = local_map.RollingLocalMap(mb)
    lm.reset(None)
    lm.insert(t4, np.array([0, 0, 0, 1.0]), np.zeros(3))
    lm.commit(0.3)
    committed = lm.target()[:, :3].copy()
    mb.setInputSource(src)
    p3 = _product(mod, committed, src)
    assert _same_bits(_everything(p3, T), _everything(mb, T)), "map-bound target"
    d.device_free(pt); d.device_free(ps); d.device_free(body_ptr)
    for x in (bo, plain, d, lz, p2, mb, p3):
        x.close()


def test_refused_with_a_solve_in_flight(mod, data):
    g = _product(mod, data["tgt"], data["src"])
    guess = np.eye(4, dtype=np.float32)
    g.linearize(data["T"], want_H=False)
    mod[1].FastVGICP.align(g, guess, want_output=False)
    want = g.getFinalTransformation().copy()
    g.linearize(data["T"], want_H=False)
    g.align_begin(guess)
    for refused in (lambda: g.linearize(data["T"]), lambda: g.compute_error(data["T"]), lambda: g.align(guess, want_output=False),
                    lambda: g.num_correspondences, lambda: g.correspondences()):
        with pytest.raises(mod[0].RgcError):
            refused()
    assert np.array_equal(g.align_end(), want)
    g.linearize(data["T"], want_H=False)
    g.close()


# ---- whole solves -------------------------------------------------------------------------------------------------------------------------
def _pose_error(X, T):
    d = np.asarray(X, np.float64) @ np.linalg.inv(T)
    return float(np.linalg.norm(d[:3, 3] - (np.eye(3) - d[:3, :3]) @ np.array(CENTER))), float(np.abs(d[:3, :3] - np.eye(3)).max())


@pytest.mark.parametrize("d_max", [None, 0.1])
def test_whole_solves(mod, data, d_max):
    tgt, src, T = data["tgt"], data["src"], data["T"]
    g = _product(mod, tgt, src, d_max=d_max)
    ref = _reference(g, tgt, src, gr.FLT_MAX if d_max is None else d_max)
    kw = dict(max_iterations=g._p.max_iterations, lm_max_iterations=g._p.lm_max_iterations, rotation_eps=g._p.rotation_eps,
              translation_eps=g._p.translation_eps, init_lambda_factor=g._p.lm_init_lambda_factor)
    rng = np.random.default_rng(3)
    for guess in (np.eye(4), nr.random_pose(rng, max_t=0.05, max_deg=0.5, about=CENTER) @ T):
        g32 = guess.astype(np.float32)
        X, iters, conv, failed, Hfin = ref.align(g32, **kw)
        kept_ref = ref.num_kept()
        X2 = ref.align(g32, perturb=1e-9, **kw)[0]
        spread = float(np.abs(X - X2).max())
        tol = max(10 * spread, nn.t_tolerance(X))
        g.align(g32, want_output=False, want_fitness=True)
        got = g.getFinalTransformation()
        diff = float(np.abs(got.astype(np.float64) - X).max())
        et, er = _pose_error(got, T)
        rt, rr = _pose_error(X, T)
        print("d_max %s: %d iterations (reference %d), converged %d/%d; |T - T_ref| = %.3g, tolerance %.3g (reference spread under a 1e-9 guess change %.3g); "
              "pose error %.4f m (reference %.4f m); kept %d of %d"
              % (d_max, g.nr_iterations, iters, g.hasConverged(), conv, diff, tol, spread, et, rt, g.num_correspondences, len(src)))
        assert (g.nr_iterations, g.hasConverged(), g.lm_failed) == (iters, conv, failed)
        assert conv and not failed
        assert diff <= tol
        assert et <= rt + 2 * tol and er <= rr + 2 * tol           # the known pose is recovered to the accuracy the reference reaches
        assert np.abs(g.getFinalHessian() - Hfin).max() <= REL * np.abs(Hfin).max()
        assert g.num_correspondences == kept_ref
        if d_max is None:
            assert kept_ref == len(src)
        else:
            assert 1000 <= kept_ref <= len(src) - 100                # counted by the reference alone (about 5170 of 8000 at 0.1 m)
        assert g.getFitnessScore() == pytest.approx(nn.score(tgt, src, got), rel=nn.sum_reorder_bound(len(src)))
    g.close()


def test_no_pair_at_all(mod, data):
    """a maximum distance no pair meets: cost 0, H = 0, b = 0, no pair; the solve ends as the voxel solve ends on an empty system (a source no voxel of
    the target holds): the same flags, the guess returned"""
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = [500.0, 500.0, 50.0]
    g = _product(mod, data["tgt"], data["src"], d_max=1e-6)
    y, H, b = g.linearize(np.eye(4))
    assert y == 0.0 and not H.any() and not b.any() and g.num_correspondences == 0
    idx, key = g.correspondences()
    assert (idx == -1).all() and (key > 0).all()
    assert g.compute_error(data["T"]) == 0.0
    mod[1].FastVGICP.align(g, far, want_output=False)
    flags = (g.hasConverged(), g.lm_failed)
    vg = g.getFinalTransformation().copy()
    g.align(far, want_output=False)
    print("empty system: voxel solve (converged, lm_failed) = %s, GICP %s" % (flags, (g.hasConverged(), g.lm_failed)))
    assert (g.hasConverged(), g.lm_failed) == flags
    assert np.array_equal(np.isfinite(vg), np.isfinite(g.getFinalTransformation()))
    g.close()


def test_cpp_mirror_runs(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "rgc-slam_amd")
    exe = tmp_path / "test_gicp"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(root, "tests", "cpp", "test_gicp.cpp"), "-o", str(exe),
                           "-L", pkg, "-lrgc_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
