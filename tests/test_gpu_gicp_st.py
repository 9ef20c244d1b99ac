"""FastGICPSingleThread (rgc_gicpst_*) on the MI355X against the independent numpy reference tests/gicp_st_reference.py, on the designed cases of
tests/gicp_st_cases.py and on whole solves.

After EVERY linearisation of a case's pose sequence the `searched` mask, idx, key1 and key2 are compared index for index and bit for bit, num_searched
and num_correspondences for equality, and cost / H / b within the relative bar tests/test_gpu_gicp.py uses for FastGICP's same terms (1e-5: of the value
for the cost, of the largest entry for H and b), the reference fed the product's own covariances from its getters.  Each test prints the measured
difference next to the reference's difference from itself when it sums in descending order.  Measured on an MI355X (EXPERIMENTS.md, round 19): at
most 6.2e-14 over all cases, the reference's own spread at most 1.5e-15.

Two cases of the issue cannot be constructed, for the reason tests/test_gpu_gicp.py gives: the context's clouds need at least k points and k >= 2, so
a SOURCE of one point and a TARGET of one point are refused (test_one_point_clouds_are_refused asserts that); key2 = +INF on a one-point target is held
by the reference alone (tests/test_gicp_st_reference.py)."""
import os
import subprocess

import numpy as np
import pytest

import gicp_reference as gr
import gicp_st_cases as cases
import gicp_st_reference as sr
import ndt_reference as nr
import nn_reference as nn

pytestmark = pytest.mark.gpu

CENTER = (100.0, -60.0, 2.0)
REL = 1e-5          # tests/test_gpu_gicp.py, REL: the same (C_B + R C_A R^T)^-1 terms


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import gicp, registration
    return gicp, registration


@pytest.fixture(scope="module")
def scene():
    """a 6 k map, a 1.5 k scan of it seen from a pose within 0.3 m / 3 deg (1 cm of noise), and that pose"""
    rng = np.random.default_rng(9102)
    tgt = nr.scene(rng, 6000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (nr.scene(rng, 1500).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (1500, 3))).astype(np.float32)
    return dict(tgt=tgt, src=src, T=T)


def _product(mod, tgt, src, k=20, d_max=None, cov_t=None, cov_s=None, method=None):
    g = mod[0].FastGICPSingleThread(0)
    g.setCorrespondenceRandomness(k)
    if method is not None:
        g.setRegularizationMethod(method)
    if d_max is not None:
        g.setMaxCorrespondenceDistance(d_max)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    if cov_t is not None:
        g.setTargetCovariances(cov_t)
    if cov_s is not None:
        g.setSourceCovariances(cov_s)
    return g


def _case_product(mod, case):
    return _product(mod, case["tgt"], case["src"], k=2, d_max=case["d_max"], cov_t=case["cov_t"], cov_s=case["cov_s"])


def _reference(g, tgt, src, d_max=sr.FLT_MAX):
    ref = sr.GICPST(d_max)
    ref.set_target(tgt, g.getTargetCovariances())
    ref.set_source(src, g.getSourceCovariances())
    return ref


def _rel(y, H, b, yr, Hr, br):
    return (abs(y - yr) / max(abs(yr), 1e-300), np.abs(H - Hr).max() / max(np.abs(Hr).max(), 1e-300), np.abs(b - br).max() / max(np.abs(br).max(), 1e-300))


def _same_state(g, ref, label):
    idx, k1, k2, was = g.correspondences()
    st = ref.state
    bad = np.flatnonzero((was != st["searched"]) | (idx != st["corr"]) | (k1 != st["key1"]) | (k2 != st["key2"]))
    assert bad.size == 0, (label, bad[:8], was[bad[:8]], st["searched"][bad[:8]], idx[bad[:8]], st["corr"][bad[:8]], k1[bad[:8]], st["key1"][bad[:8]],
                           k2[bad[:8]], st["key2"][bad[:8]])
    assert g.num_searched() == ref.num_searched() and g.num_correspondences == ref.num_kept(), label


def _step(g, ref, T, label):
    """one linearisation of both at T, everything compared; returns (worst relative difference, the reference's own spread)"""
    y, H, b = g.linearize(T)
    yr, Hr, br = ref.linearize(T)
    _same_state(g, ref, label)
    if ref.num_kept() == 0:
        assert y == 0.0 and not H.any() and not b.any()
        return 0.0, 0.0
    errs = _rel(y, H, b, yr, Hr, br)
    spread = max(_rel(*ref.sums(T, descending=True), yr, Hr, br))
    assert max(errs) <= REL, (label, errs)
    assert np.array_equal(H, H.T)
    assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
    T3 = cases.translation(0.01, -0.02, 0.005) @ T
    e, er = g.compute_error(T3), ref.compute_error(T3)
    assert abs(e - er) <= REL * abs(er), (label, e, er)
    _same_state(g, ref, label + " (after compute_error)")                     # the frozen cost leaves the state alone
    return max(max(errs), abs(e - er) / abs(er)), spread


def _run_case(mod, case, each=None):
    g = _case_product(mod, case)
    ref = _reference(g, case["tgt"], case["src"], case["d_max"])
    assert np.abs(ref.cov_t - case["cov_t"]).max() <= 2e-9 and np.abs(ref.cov_s - case["cov_s"]).max() <= 2e-9
    worst = spread = 0.0
    searched = []
    for i, step in enumerate(case["steps"]):
        if isinstance(step, str):
            g.reset()
            ref.reset()
            continue
        w, s = _step(g, ref, step, "%s step %d" % (case["name"], i))
        worst, spread = max(worst, w), max(spread, s)
        searched.append(g.num_searched())
        if each:
            each(g, ref, step)
    print("%s: searched per step %s of %d; product - reference %.3g relative, reference - itself (descending sum) %.3g; bound %.1g"
          % (case["name"], searched, len(case["src"]), worst, spread, REL))
    g.close()
    return searched


# ---- the designed cases: every linearisation of every pose sequence ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SIZES)
def test_source_sizes_at_the_compaction_edges(mod, n):
    searched = _run_case(mod, cases.sizes_case(n))
    assert searched[0] == n and searched[1] == 0 and 0 < searched[2] < n and searched[3] == n


def test_one_point_clouds_are_refused(mod):
    case = cases.sizes_case(63)
    for tgt, src in ((case["tgt"][:1], case["src"]), (case["tgt"], case["src"][:1])):
        g = mod[0].FastGICPSingleThread(0)
        g.setCorrespondenceRandomness(2)
        with pytest.raises(mod[0].RgcError):                       # k >= 2 and a cloud of at least k points: the context's rule for every cloud
            g.setInputTarget(tgt)
            g.setInputSource(src)
        g.close()


@pytest.mark.parametrize("case", [cases.two_points_case(), cases.duplicates_case(), cases.lattice_ties_case()], ids=lambda c: c["name"])
def test_tiny_and_tied_targets(mod, case):
    searched = _run_case(mod, case)
    if case["name"] != "two_points":
        assert searched == [len(case["src"])] * len(searched)       # key1 == key2: never skipped


@pytest.mark.parametrize("case", [cases.walls_case(), cases.outside_case(), cases.sparse_case()], ids=lambda c: c["name"])
def test_second_nearest_against_brute_force(mod, case):
    _run_case(mod, case)


def test_threshold_stickiness(mod):
    corr = []
    _run_case(mod, cases.sticky_case(), lambda g, ref, T: corr.append(g.correspondences()[0].tolist()))
    assert corr == [[0, -1], [0, -1], [-1, 0]], corr                # kept at 1.1 m, -1 at 0.9 m; both flip after the reset


def test_stale_M_is_the_single_thread_cost_not_fastgicps(mod):
    case = cases.stale_case()
    g = _case_product(mod, case)
    ref = _reference(g, case["tgt"], case["src"], case["d_max"])
    T1, T2 = case["steps"]
    _step(g, ref, T1, "stale_M first")
    _step(g, ref, T2, "stale_M second")
    assert g.num_searched() == 0
    y = ref.sums(T2)[0]
    plain = mod[0].FastGICP.linearize(g, T2, want_H=False)[0]      # rgc_gicp_linearize on the same context: the same pairs, M recomputed at T2
    print("stale_M: single-thread cost %.6g (reference), FastGICP's at the same pose %.6g: relative difference %.3g" % (y, plain, abs(y - plain) / abs(plain)))
    assert abs(y - plain) >= 100 * REL * abs(plain)
    _same_state(g, ref, "stale_M after rgc_gicp_linearize")          # FastGICP's calls on the same context leave this state alone
    g.close()


# ---- the state's life ---------------------------------------------------------------------------------------------------------------------------
def test_what_drops_the_anchors(mod, scene):
    tgt, src, T = scene["tgt"], scene["src"], scene["T"]
    n = len(src)
    g = _product(mod, tgt, src)
    for refused in (lambda: g.compute_error(T), lambda: g.num_searched(), lambda: g.num_correspondences, lambda: g.correspondences()):
        with pytest.raises(mod[0].RgcError) as e:
            refused()                                               # no linearisation yet
        assert e.value.status == -1
    drops = [g.reset, lambda: g.setInputSource(src), lambda: g.setInputTarget(tgt), lambda: g.setSourceCovariances(g.getSourceCovariances()),
             lambda: g.setTargetCovariances(g.getTargetCovariances()), lambda: (g.swapSourceAndTarget(), g.swapSourceAndTarget()),
             lambda: (g.clearSource(), g.setInputSource(src)), lambda: (g.clearTarget(), g.setInputTarget(tgt))]
    for drop in drops:
        g.linearize(T, want_H=False)
        y = g.linearize(T, want_H=False)[0]
        assert g.num_searched() < n // 2                            # anchors in force: at the same pose only tied points are searched
        assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
        drop()
        for refused in (lambda: g.compute_error(T), lambda: g.num_searched(), lambda: g.correspondences()):
            with pytest.raises(mod[0].RgcError):
                refused()
        g.linearize(T, want_H=False)
        assert g.num_searched() == n                                # dropped: every point searched
    g.linearize(T, want_H=False)
    before = g.num_searched()
    g.setMaxCorrespondenceDistance(0.05)                            # a new gate drops nothing ...
    y = g.compute_error(T)
    kept = g.num_correspondences
    g.linearize(T, want_H=False)
    assert g.num_searched() == before and g.num_correspondences == kept     # ... and a skipped point keeps the pair the old gate gave it
    assert g.compute_error(T) == pytest.approx(y, rel=1e-13)
    g.reset()
    g.linearize(T, want_H=False)
    assert g.num_searched() == n and g.num_correspondences < kept
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
    g.close()


def test_refused_with_a_solve_in_flight(mod, scene):
    g = _product(mod, scene["tgt"], scene["src"])
    guess = np.eye(4, dtype=np.float32)
    g.linearize(scene["T"], want_H=False)
    g.align_begin(guess)
    for refused in (lambda: g.linearize(scene["T"]), lambda: g.compute_error(scene["T"]), lambda: g.align(guess, want_output=False), g.reset,
                    lambda: g.num_correspondences, lambda: g.num_searched(), lambda: g.correspondences()):
        with pytest.raises(mod[0].RgcError):
            refused()
    g.align_end()
    g.linearize(scene["T"], want_H=False)
    g.close()


def _sequence(g, T):
    """a pose sequence (first, the same again, a small step, reset, a larger step) and everything the product gives after each"""
    out = []
    steps = [T, T, cases.translation(0.03, -0.02, 0.01) @ T, "reset", cases.translation(0.4, 0.3, -0.1) @ T, T]
    for s in steps:
        if isinstance(s, str):
            g.reset()
            continue
        y, H, b = g.linearize(s)
        out.append((np.float64(y), H, b) + g.correspondences() + (np.int64(g.num_searched()), np.int64(g.num_correspondences),
                                                                  np.float64(g.compute_error(cases.translation(0.01, 0.0, 0.0) @ s))))
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for u, v in zip(a, b) for x, y in zip(u, v))


def test_routes_give_identical_bits(mod, scene):
    tgt, src, T = scene["tgt"], scene["src"], scene["T"]
    plain = _product(mod, tgt, src)
    base = _sequence(plain, T)
    assert base[0][7] == len(src) and base[1][7] < len(src) and base[2][7] < len(src) and base[3][7] == len(src)   # the cached route was taken
    plain.reset()
    assert _same_bits(base, _sequence(plain, T)), "two runs"
    # the reference on this sequence's first steps
    ref = _reference(plain, tgt, src)
    plain.reset()
    for i, s in enumerate((T, T, cases.translation(0.03, -0.02, 0.01) @ T)):
        _step(plain, ref, s, "scene step %d" % i)
    # device pointers
    d = mod[0].FastGICPSingleThread(0)
    t4, s4 = np.zeros((len(tgt), 4), np.float32), np.zeros((len(src), 4), np.float32)
    t4[:, :3], s4[:, :3] = tgt, src
    pt, ps = d.device_alloc(t4.nbytes), d.device_alloc(s4.nbytes)
    d.upload(pt, t4); d.upload(ps, s4)
    d.setInputTargetDevice(pt, len(tgt), 16); d.setInputSourceDevice(ps, len(src), 16)
    assert _same_bits(base, _sequence(d, T)), "device pointers"
    # lazy target (completed first)
    lz = mod[0].FastGICPSingleThread(0)
    lz.setLazyTarget(2)
    lz.setInputTarget(tgt); lz.setInputSource(src)
    assert _same_bits(base, _sequence(lz, T)), "lazy target"
    lz.close()
    # borrowed target
    bo = mod[0].FastGICPSingleThread(0)
    bo.shareTargetFrom(plain)
    bo.setInputSource(src)
    assert _same_bits(base, _sequence(bo, T)), "borrowed target"
    # re-framed target: compared with a plain target of the re-framed points
    body_ptr = d.device_alloc(t4.nbytes)
    q, t = np.array([0.0, 0.0, np.sin(0.05), np.cos(0.05)]), np.array([0.3, -0.2, 0.01])
    d.setInputTargetReframed(pt, len(tgt), 16, q, t, body_ptr)
    body = d.download(body_ptr, (len(tgt), 4))[:, :3].copy()
    rf = _sequence(d, T)
    p2 = _product(mod, body, src)
    assert _same_bits(_sequence(p2, T), rf), "re-framed target"
    d.linearize(T, want_H=False)
    d.setInputTargetReframed(pt, len(tgt), 16, q, t, body_ptr)       # a new frame drops the anchors
    d.linearize(T, want_H=False)
    assert d.num_searched() == len(src)
    d.device_free(pt); d.device_free(ps); d.device_free(body_ptr)
    for x in (bo, plain, d, p2):
        x.close()


# ---- whole solves ---------------------------------------------------------------------------------------------------------------------------------
def _gen_scene(mod):
    rng = np.random.default_rng(9103)
    tgt = nr.scene(rng, 6000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (nr.scene(rng, 1500).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (1500, 3))).astype(np.float32)
    return tgt, src, np.eye(4), dict(k=20)


def _gen_volume(mod):
    rng = np.random.default_rng(9104)
    tgt = (rng.uniform(-4, 4, (6000, 3)) + np.array(CENTER)).astype(np.float32)
    T = nr.random_pose(rng, max_t=0.1, max_deg=1.0, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (tgt[::4].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.02, (1500, 3))).astype(np.float32)
    return tgt, src, np.eye(4), dict(k=20, method=mod[1].FastVGICP.REG_FROBENIUS)      # the general covariance route


def _gen_synth(mod):
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(6000, seed=synth.SEED)
    T_true = synth.se3(synth.rot_zyx(0.02, 0.002, -0.001), [0.12, 0.02, 0.001])
    src = synth.make_scan_n(world, T_true, 1500, seed=synth.SEED)["xyz"]
    return np.asarray(tgt, np.float32)[:, :3], np.asarray(src, np.float32)[:, :3], np.eye(4), dict(k=20, d_max=1.0)


@pytest.mark.parametrize("gen", [_gen_scene, _gen_volume, _gen_synth], ids=["scene", "volume_general_route", "synth_scan_d_max_1"])
def test_whole_solves(mod, gen):
    tgt, src, guess, kw_p = gen(mod)
    g = _product(mod, tgt, src, **kw_p)
    ref = _reference(g, tgt, src, kw_p.get("d_max", sr.FLT_MAX))
    kw = dict(max_iterations=g._p.max_iterations, lm_max_iterations=g._p.lm_max_iterations, rotation_eps=g._p.rotation_eps,
              translation_eps=g._p.translation_eps, init_lambda_factor=g._p.lm_init_lambda_factor)
    g32 = guess.astype(np.float32)
    X, iters, conv, failed, Hfin = ref.align(g32, **kw)
    series, poses, kept_ref = list(ref.series), list(ref.poses), ref.num_kept()
    X2 = ref.align(g32, perturb=1e-9, **kw)[0]
    spread = float(np.abs(X - X2).max())
    tol = max(10 * spread, nn.t_tolerance(X))                       # tests/test_gpu_gicp.py, test_whole_solves: the same margin
    g.linearize(np.eye(4), want_H=False)                            # a state from before the solve: rgc_gicpst_align must drop it
    g.align(g32, want_output=False)
    got, H1, flags = g.getFinalTransformation().copy(), g.getFinalHessian().copy(), (g.nr_iterations, g.hasConverged(), g.lm_failed)
    last_searched, kept = g.num_searched(), g.num_correspondences
    g.align(g32, want_output=False)                                 # again, over the first solve's state: identical
    assert np.array_equal(got, g.getFinalTransformation()) and np.array_equal(H1, g.getFinalHessian())
    assert flags == (g.nr_iterations, g.hasConverged(), g.lm_failed) and last_searched == g.num_searched()
    diff = float(np.abs(got.astype(np.float64) - X).max())
    print("%d iterations (reference %d), converged %d/%d, lm_failed %d/%d; |T - T_ref| = %.3g, tolerance %.3g (reference spread under a 1e-9 guess change %.3g); "
          "searched per linearisation (reference) %s of %d; kept %d" % (flags[0], iters, flags[1], conv, flags[2], failed, diff, tol, spread, series, len(src), kept))
    assert flags == (iters, conv, failed)
    assert diff <= tol
    assert np.abs(H1 - Hfin).max() <= REL * np.abs(Hfin).max()
    assert kept == kept_ref and last_searched == series[-1]
    assert series[0] == len(src) and (len(series) < 2 or min(series[1:]) < len(src))
    # the series itself: the product replays the reference's linearisation poses from a reset
    g.reset()
    replay = []
    for T in poses:
        g.linearize(T, want_H=False)
        replay.append(g.num_searched())
    assert replay == series
    g.close()


def test_cpp_mirror_runs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "rgc-slam_amd")
    exe = tmp_path / "test_gicp_st"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(root, "tests", "cpp", "test_gicp_st.cpp"), "-o", str(exe),
                           "-L", pkg, "-lrgc_hip", "-Wl,-rpath," + pkg])
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
