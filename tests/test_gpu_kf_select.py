"""The keyframe store's travelled distance and the mapping node's three selections on the GPU (rgc_kf_get_travel, rgc_kf_select_surrounding / _global,
rgc_kf_detect_loop, through rgc_slam_amd.keyframes) against tests/us_reference.py on the designed drives of tests/us_cases.py.  -m gpu.
Every comparison is exact: ids, counts, fp32 travel values and radii as bit patterns.  The census minima of the cases are checked without a GPU by
tests/test_us_reference.py and again here where a case depends on them."""
import ctypes as C

import numpy as np
import pytest

import us_cases as uc
import us_reference as us
from rgc_slam_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = -1
_ip = C.POINTER(C.c_int)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def make_store(poses, ids, features=True):
    from rgc_slam_amd import keyframes
    s = keyframes.KeyframeStore()
    for p, i in zip(poses, ids):
        c = uc.tiny_cloud(i)
        s.push(int(i), p, c if features else None, c[:2] if features else None, c)
    return s


def route_of(store):
    r = _lib.VgRoute()
    assert store._L.rgc_voxelgrid_route(store._h, C.byref(r)) == 0
    return {k: (list(getattr(r, k)) if k in ("minb", "div") else int(getattr(r, k))) for k, _ in _lib.VgRoute._fields_}


@pytest.fixture(scope="module")
def drive5000():
    poses, ids = uc.lattice_drive(5000)
    s = make_store(poses, ids)
    yield s, poses, ids
    s.close()


@pytest.fixture(scope="module")
def square():
    poses, ids = uc.square_drive()
    s = make_store(poses, ids)
    d, _ = us.travel(poses)
    yield s, poses, ids, d
    s.close()


def test_travel_bit_for_bit_with_corrections_and_reset():
    """after pushes; after set_poses in between (the next push measures from the CORRECTED pose, the values already stored stay); after reset"""
    from rgc_slam_amd import keyframes
    rng = np.random.default_rng(5)
    poses = np.cumsum(rng.normal(0, 0.4, (120, 6)), axis=0).astype(F)
    poses[:, 5] = ((poses[:, 5] * 3 + np.pi) % (2 * np.pi) - np.pi).astype(F)
    ids = (2 * np.arange(120) + 3).astype(np.int32)
    s = keyframes.KeyframeStore()
    try:
        d0, a0 = s.travel([])
        assert len(d0) == 0
        for p, i in zip(poses[:60], ids[:60]):
            s.push(int(i), p, uc.tiny_cloud(i))
        wd, wa = us.travel(poses[:60])
        d, a = s.travel(ids[:60])
        assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(a), bits(wa)) and d[0] == 0 and a[0] == 0
        corrected = poses[:60].copy()
        corrected[:, :3] += np.array([0.7, -0.3, 0.1], F) * np.linspace(0, 1, 60)[:, None].astype(F)
        corrected[:, 5] += F(0.2)
        s.set_poses(ids[:60], corrected)
        d, a = s.travel(ids[:60])
        assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(a), bits(wa)), "never recomputed"
        wd, wa = list(wd), list(wa)
        stored = corrected[-1]
        for k in range(60, 120):
            s.push(int(ids[k]), poses[k], uc.tiny_cloud(ids[k]))
            x, y = us.travel_step(wd[-1], wa[-1], stored, poses[k])
            wd.append(x); wa.append(y)
            stored = poses[k]
        d, a = s.travel(ids)
        assert np.array_equal(bits(d), bits(np.array(wd, F))) and np.array_equal(bits(a), bits(np.array(wa, F)))
        plain = us.travel(poses)[0]
        assert d[60] != plain[60], "the step after the correction is measured from the corrected pose"
        only_d = np.zeros(3, F)
        q = np.ascontiguousarray(ids[[7, 3, 7]])
        assert s._L.rgc_kf_get_travel(s._h, q.ctypes.data_as(_ip), 3, only_d.ctypes.data_as(C.POINTER(C.c_float)), None) == 0
        assert np.array_equal(bits(only_d), bits(d[[7, 3, 7]]))
        with pytest.raises(_lib.RgcError):
            s.travel([4])
        s.reset()
        for p, i in zip(poses[40:50], ids[40:50]):
            s.push(int(i), p, uc.tiny_cloud(i))
        d, a = s.travel(ids[40:50])
        wd, wa = us.travel(poses[40:50])
        assert np.array_equal(bits(d), bits(wd)) and np.array_equal(bits(a), bits(wa)) and d[0] == 0
    finally:
        s.close()


def test_gate_is_strict():
    """key poses at (3, 4, 0) and (9, 12, 0) from the query with radius 5 and 15: d2 == r2, outside; the adjacent fp32 value inside"""
    q = np.array([1.0, -2.0, 0.5], F)
    offs = np.array([[3, 4, 0], [3, np.nextafter(F(4), F(0)), 0], [9, 12, 0], [9, np.nextafter(F(12), F(0)), 0], [0.25, 0, 0], [20, 0, 0]], F)
    poses = np.zeros((len(offs), 6), F)
    poses[:, :3] = q + offs
    ids = np.array([11, 12, 13, 14, 15, 16], np.int32)
    s = make_store(poses, ids)
    try:
        for radius, want in ((5.0, [12, 15]), (15.0, [11, 12, 14, 15])):
            inside, d2, r2 = us.gate(poses[:, :3], q, radius)
            assert sorted(ids[inside]) == want and (d2 == r2).sum() == 1
            got, n_in = s.select_surrounding(q, radius, 0.05, return_count=True)
            w_ids, w_n, _ = us.select_surrounding(poses[:, :3], ids, q, radius, 0.05)
            assert n_in == w_n == len(want) and list(got) == list(w_ids) and sorted(got) == want
            assert route_of(s)["chain"] == 1 and route_of(s)["n"] == n_in
        got, n_in = s.select_surrounding(q + np.array([100, 0, 0], F), 5.0, 0.3, return_count=True)
        assert len(got) == 0 and n_in == 0
    finally:
        s.close()


@pytest.mark.parametrize("n", [1, 2, 65])
def test_small_stores(n):
    poses, ids = uc.lattice_drive(n)
    s = make_store(poses, ids)
    try:
        for density in (0.5, 0.3):
            w, _ = us.select_global(poses[:, :3], ids, density)
            assert list(s.select_global(density)) == list(w)
            r = route_of(s)
            assert (r["chain"], r["n"], r["n_out"], r["status"]) == (1, n, len(w), 0), r
            centre = poses[n // 2, :3] + np.array([0.03, 0.02, 0.0], F)
            w, w_n, _ = us.select_surrounding(poses[:, :3], ids, centre, 3.0, density)
            got, n_in = s.select_surrounding(centre, 3.0, density, return_count=True)
            assert n_in == w_n and list(got) == list(w)
    finally:
        s.close()


def test_surrounding_and_global_on_5000_keyframes(drive5000):
    """a serpentine lattice drive with a planted exact tie in every full leaf; ids are not positions; twice each: bit-identical from run to run"""
    s, poses, ids = drive5000
    for density in (0.5, 0.3):
        w, g = us.select_global(poses[:, :3], ids, density)
        if density == 0.5:
            assert g.census()["tie_leaves"] >= 20 and (g.index != g.first).sum() >= 100
        for k in range(2):
            assert np.array_equal(s.select_global(density), w), (density, k)
            r = route_of(s)
            assert (r["chain"], r["n"], r["n_out"], r["status"]) == (1, 5000, len(w), 0), r     # (which buckets: the kept box of this leaf size decides)
    for centre, radius in ((poses[2500, :3] + np.array([0.03, 0.02, 0.0], F), 3.0), (np.array([0.0, 0.0, 0.0], F), 15.0), (poses[77, :3], 0.4)):
        for density in (0.5, 0.3):
            w, w_n, u = us.select_surrounding(poses[:, :3], ids, centre, radius, density)
            for k in range(2):
                got, n_in = s.select_surrounding(centre, radius, density, return_count=True)
                assert n_in == w_n and np.array_equal(got, w), (centre, radius, density, k)
                r = route_of(s)
                assert (r["chain"], r["n"], r["n_out"]) == (1, w_n, len(w)), r
    w, w_n, u = us.select_surrounding(poses[:, :3], ids, poses[2500, :3] + np.array([0.03, 0.02, 0.0], F), 3.0, 0.5)
    assert 0 < w_n < 5000 and u.census()["tie_leaves"] >= 20


def test_revision_moves_the_mirror(drive5000):
    """set_poses between two selections: the second sees the new positions"""
    s, poses, ids = drive5000
    moved = poses.copy()
    moved[100:200, :3] += np.array([0.0, 40.0, 0.0], F)
    try:
        before = s.select_global(0.5)
        s.set_poses(ids[100:200], moved[100:200])
        w, _ = us.select_global(moved[:, :3], ids, 0.5)
        got = s.select_global(0.5)
        assert np.array_equal(got, w) and not np.array_equal(got, before)
    finally:
        s.set_poses(ids[100:200], poses[100:200])
    assert np.array_equal(s.select_global(0.5), before)


def test_cap_one_short_and_bad_arguments(drive5000):
    s, poses, ids = drive5000
    L, h = s._L, s._h
    w, _ = us.select_global(poses[:, :3], ids, 0.5)
    out = np.full(5000, -9, np.int32)
    no, nin = C.c_int(-1), C.c_int(-1)
    assert L.rgc_kf_select_global(h, 0.5, out.ctypes.data_as(_ip), len(w) - 1, C.byref(no)) == ERR_INVALID
    assert no.value == len(w) and (out == -9).all()
    assert L.rgc_kf_select_global(h, 0.5, out.ctypes.data_as(_ip), len(w), C.byref(no)) == 0 and np.array_equal(out[:len(w)], w)
    centre = np.array([3.0, 3.0, 0.0], F)
    w, w_n, _ = us.select_surrounding(poses[:, :3], ids, centre, 3.0, 0.5)
    out[:] = -9
    fp = C.POINTER(C.c_float)
    assert L.rgc_kf_select_surrounding(h, centre.ctypes.data_as(fp), 3.0, 0.5, out.ctypes.data_as(_ip), len(w) - 1, C.byref(nin), C.byref(no)) == ERR_INVALID
    assert (nin.value, no.value) == (w_n, len(w)) and (out == -9).all()
    for radius, density in ((0.0, 0.5), (-1.0, 0.5), (np.nan, 0.5), (np.inf, 0.5), (3.0, 0.0), (3.0, -0.5), (3.0, np.nan)):
        assert L.rgc_kf_select_surrounding(h, centre.ctypes.data_as(fp), radius, density, out.ctypes.data_as(_ip), 5000, C.byref(nin), C.byref(no)) == ERR_INVALID
    bad = np.array([np.nan, 0, 0], F)
    assert L.rgc_kf_select_surrounding(h, bad.ctypes.data_as(fp), 3.0, 0.5, out.ctypes.data_as(_ip), 5000, C.byref(nin), C.byref(no)) == ERR_INVALID
    for density in (0.0, -1.0, np.nan, np.inf):
        assert L.rgc_kf_select_global(h, density, out.ctypes.data_as(_ip), 5000, C.byref(no)) == ERR_INVALID
    got, n_in = s.select_surrounding(centre, 3.0, 0.5, return_count=True)
    assert n_in == w_n and np.array_equal(got, w)


def test_empty_store():
    from rgc_slam_amd import keyframes
    s = keyframes.KeyframeStore()
    try:
        assert len(s.select_global(0.5)) == 0 and len(s.select_surrounding([0, 0, 0], 15.0, 0.3)) == 0
        d = s.detect_loop()
        assert not d["found"] and len(d["history_ids"]) == 0 and d["latest_id"] == -1
    finally:
        s.close()


def _same_loop(got, want):
    assert got["found"] == want["found"] and got["latest_id"] == want["latest_id"] and got["closest_id"] == want["closest_id"], (got, want)
    assert got["n_in_radius"] == want["n_in_radius"] and list(got["history_ids"]) == want["history_ids"], (got, want)
    assert F(got["search_radius"]).view(np.uint32) == F(want["search_radius"]).view(np.uint32)


def test_loop_on_the_square_drive(square):
    """248 keyframes at 0.5 m around a 30 m square, re-entering the first side: the nearest qualifying poses have ids below min_key_id and are skipped"""
    s, poses, ids, d = square
    nf = np.full(len(ids), 6)
    assert np.array_equal(bits(s.travel(ids)[0]), bits(d))
    want = us.detect_loop(poses[:, :3], ids, d, nf)
    assert want == us.detect_loop_literal(poses[:, :3], ids, d, nf)
    assert want["found"] and want["closest_id"] == 10 and want["nearer_skipped_for_id"] >= uc.SQUARE_MINIMA["nearer_skipped_for_id"]
    assert want["n_in_radius"] >= uc.SQUARE_MINIMA["n_in_radius"] and want["history_ids"] == list(range(61))          # the window is clipped at 0
    for k in range(2):
        got = s.detect_loop()
        _same_loop(got, want)
        assert np.array_equal(bits(got["latest_pose"]), bits(poses[247])) and np.array_equal(bits(got["closest_pose"]), bits(poses[10]))
    cases = (dict(history_search_num=300),               # the window is clipped at L (and by id < latest id)
             dict(history_search_num=0), dict(distance_by_loop=-5000.0), dict(history_search_radius=-10.0), dict(min_key_id=0), dict(min_key_id=22),
             dict(loop_keyframe_dis_diff=200.0), dict(drift_factor=0.0, history_search_radius=0.3))
    seen = set()
    for kw in cases:
        want = us.detect_loop(poses[:, :3], ids, d, nf, **kw)
        assert want == us.detect_loop_literal(poses[:, :3], ids, d, nf, **kw)
        _same_loop(s.detect_loop(**kw), want)
        seen.add((want["found"], want["closest_id"] >= 0))
    assert us.detect_loop(poses[:, :3], ids, d, nf, history_search_num=300)["history_ids"] == list(range(247))
    assert not us.detect_loop(poses[:, :3], ids, d, nf, distance_by_loop=-5000.0)["found"]
    assert us.detect_loop(poses[:, :3], ids, d, nf, history_search_radius=-10.0)["search_radius"] < 0
    assert seen == {(True, True), (False, False)}
    # cap one short: the counts are reported, nothing is written
    prm = _lib.KfLoopParams()
    s._L.rgc_default_kf_loop_params(C.byref(prm))
    hist, cand, nh = np.full(100, -9, np.int32), _lib.KfLoopCandidate(), C.c_int(-1)
    assert s._L.rgc_kf_detect_loop(s._h, C.byref(prm), C.byref(cand), hist.ctypes.data_as(_ip), 60, C.byref(nh)) == ERR_INVALID
    assert nh.value == 61 and (hist == -9).all() and cand.found == 0
    assert s._L.rgc_kf_detect_loop(s._h, C.byref(prm), C.byref(cand), hist.ctypes.data_as(_ip), 61, C.byref(nh)) == 0 and cand.found == 1
    prm.drift_factor = float("nan")
    assert s._L.rgc_kf_detect_loop(s._h, C.byref(prm), C.byref(cand), hist.ctypes.data_as(_ip), 100, C.byref(nh)) == ERR_INVALID


def test_loop_ids_that_are_not_positions_and_bare_history():
    poses, pos = uc.square_drive()
    d, _ = us.travel(poses)
    ids = (3 * pos + 1).astype(np.int32)
    s = make_store(poses, ids)
    try:
        want = us.detect_loop(poses[:, :3], ids, d, np.full(len(ids), 6))
        assert want["found"] and want["closest_pos"] == 7 and want["closest_id"] == 22
        _same_loop(s.detect_loop(), want)
    finally:
        s.close()
    s = make_store(poses, pos, features=False)                       # scans only: the history holds no corner or surf point
    try:
        want = us.detect_loop(poses[:, :3], pos, d, np.zeros(len(pos), int))
        assert not want["found"] and want["closest_id"] == 10 and len(want["history_ids"]) == 61
        _same_loop(s.detect_loop(), want)
    finally:
        s.close()
    shuffled = np.random.default_rng(3).permutation(len(pos)).astype(np.int32)      # ids in no order: the id filters of the window bite
    s = make_store(poses, shuffled)
    try:
        want = us.detect_loop(poses[:, :3], shuffled, d, np.full(len(pos), 6), min_key_id=0)
        assert want == us.detect_loop_literal(poses[:, :3], shuffled, d, np.full(len(pos), 6), min_key_id=0) and 0 < len(want["history_ids"]) < 61
        _same_loop(s.detect_loop(min_key_id=0), want)
    finally:
        s.close()


def test_selections_leave_a_solve_in_flight_alone(square):
    """between rgc_align_begin and rgc_align_end every selection runs, returns what it returns alone, and the solve's result is bit-identical"""
    import rgc_slam_amd.synth as synth
    s, poses, ids, d = square
    L, h = s._L, s._h
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    world, base = synth.make_world_and_map(20000, seed=3)
    tgt = np.ascontiguousarray(base, F)
    src = np.ascontiguousarray(base[::3] + F(0.02), F)
    guess = np.eye(4, dtype=F)
    alone = (s.detect_loop(), s.select_global(0.5), s.select_surrounding(poses[240, :3], 15.0, 0.3), s.travel(ids))

    def solve(between):
        assert L.rgc_set_target(h, tgt.ctypes.data, len(tgt), 12) == 0 and L.rgc_set_source(h, src.ctypes.data, len(src), 12) == 0
        assert L.rgc_align_begin(h, guess.ctypes.data_as(fp), 1) == 0
        res = (s.detect_loop(), s.select_global(0.5), s.select_surrounding(poses[240, :3], 15.0, 0.3), s.travel(ids)) if between else None
        T, H, fit = np.zeros(16, F), np.zeros(36), C.c_double(0)
        it, conv, lmf = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.rgc_align_end(h, T.ctypes.data_as(fp), H.ctypes.data_as(dp), C.byref(fit), C.byref(it), C.byref(conv), C.byref(lmf)) == 0
        return (T.tobytes(), H.tobytes(), np.float64(fit.value).tobytes(), it.value, conv.value, lmf.value), res
    solve(False)
    plain, busy, again = solve(False), solve(True), solve(False)
    assert plain[0] == again[0] == busy[0] and plain[0][3] >= 1
    _same_loop(busy[1][0], dict(alone[0], history_ids=list(alone[0]["history_ids"])))
    assert np.array_equal(busy[1][1], alone[1]) and np.array_equal(busy[1][2], alone[2]) and np.array_equal(bits(busy[1][3][0]), bits(alone[3][0]))


def test_end_to_end_detected_loop_closure():
    """tests/test_gpu_pose_graph.py::test_end_to_end_loop_closure with the loop pair and both selections FOUND by the library:
    detect_loop -> assemble(latest), assemble(history) -> rgc_icp_align_device -> loop_from_icp -> optimize(apply) -> select_global -> assemble.
    The planted drift and the three bounds are that test's; what is new is asserted exactly (the detection, the global selection).  The drive is that
    test's too, sampled every 9th frame instead of every 3rd: there the key poses are 0.41 m apart and the planted drift of 0.43 m carries the revisiting pose
    past keyframe 2 to keyframe 3 -- the nearest-pose rule then (rightly) names 3.  At 1.2 m between key poses the planted pair is the nearest one."""
    import pgo_reference as ref
    from rgc_slam_amd import keyframes, pose_graph
    ids, poses, clouds = keyframes.synthetic_keyframes(24, seed=9400, every=9)
    ids = list(ids)
    truth = np.array(poses, F)
    revisit, loop = 24, ids[2]
    ids.append(revisit)
    clouds[revisit] = clouds[loop]
    truth = np.concatenate([truth, truth[2:3]])
    poses = truth.copy()
    poses[:, :3] += (np.linspace(0.0, 1.0, len(ids))[:, None] ** 2 * np.array([0.35, -0.25, 0.05])).astype(F)
    poses[:, 5] += (np.deg2rad(1.5) * np.linspace(0.0, 1.0, len(ids)) ** 2).astype(F)
    store = keyframes.KeyframeStore()
    try:
        for k, i in enumerate(ids):
            store.push(i, poses[k], *clouds[i])
        # the node's constants scaled to a 25-keyframe drive: no id floor, a window of three keyframes either side, a quarter of the drive between the pair
        d = us.travel(poses)[0]
        kw = dict(min_key_id=0, history_search_num=3, history_search_radius=1.0, loop_keyframe_dis_diff=float(d[-1]) / 4)
        nf = np.array([len(clouds[i][0]) + len(clouds[i][1]) for i in ids])
        want = us.detect_loop(poses[:, :3], np.array(ids), d, nf, **kw)
        det = store.detect_loop(**kw)
        print("detected: %s (search radius %.3f m over %.1f m travelled, %d poses inside)" % (det, det["search_radius"], d[-1], det["n_in_radius"]))
        _same_loop(det, want)
        assert det["found"] and det["latest_id"] == revisit and det["closest_id"] == loop, "the planted pair"
        assert list(det["history_ids"]) == ids[:6]
        source = store.assemble([det["latest_id"]], (keyframes.KF_CORNER, keyframes.KF_SURF), device=True)
        target = store.assemble(det["history_ids"], (keyframes.KF_CORNER, keyframes.KF_SURF), device=True)
        prm = _lib.IcpParams()
        L = store._L
        L.rgc_default_icp_params(C.byref(prm))
        T, res = np.zeros(16, F), _lib.IcpResult()
        store._chk(L.rgc_icp_align_device(store._h, source.ptr, source.n, target.ptr, target.n, 16, C.byref(prm), T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res)))
        graph = pose_graph.PoseGraph4DoF(store)
        edge = graph.loop_from_icp(det["latest_id"], det["latest_pose"], det["closest_id"], det["closest_pose"], T.reshape(4, 4))
        rep, out = graph.optimize(ids, apply=True)
        assert rep["status"] == ref.OPTIMIZED and rep["fixed_id"] == loop and rep["successful"] >= 1
        loops = [dict(key_curr=revisit, key_loop=loop, t=np.array(edge.t_loop_curr[:]), yaw=edge.yaw_loop_curr_deg, pitch=edge.pitch_loop_deg, roll=edge.roll_loop_deg)]
        g = ref.build_graph(ids, poses, loops)
        x_ref, info = ref.lm_solve(g, ref.state_of(poses)[0])
        want_p = ref.poses_of(x_ref, poses)
        rel = lambda P: P[-1, :3].astype(np.float64) - P[2, :3].astype(np.float64)          # noqa: E731
        assert not rel(truth).any()
        R2, _ = ref.ypr_matrix(float(ref.state_of(poses)[0][2, 0]), edge.pitch_loop_deg, edge.roll_loop_deg, np.float64)
        measured = R2 @ np.array(edge.t_loop_curr[:])
        ulp = 4 * float(np.spacing(F(np.abs(want_p[:, :3]).max())))
        rms = float(np.sqrt(res.fitness))
        left_by_solve = float(np.linalg.norm(rel(want_p) - measured))
        e_before, e_after = float(np.linalg.norm(rel(poses))), float(np.linalg.norm(rel(out)))
        print("end to end: loop pair error %.4f m -> %.4f m; ICP RMS residual %.4f m" % (e_before, e_after, rms))
        assert np.abs(out[:, :3].astype(np.float64) - want_p[:, :3].astype(np.float64)).max() <= ulp
        assert rms < 0.5 * e_before
        assert e_after <= rms + left_by_solve + ulp
        # the global map of the corrected store: the selection over the corrected poses, exactly; assembled through the leaf filter
        sel = store.select_global(0.5)
        w, _ = us.select_global(out[:, :3], np.array(ids), 0.5)
        assert np.array_equal(sel, w)
        gm = store.assemble(sel, (keyframes.KF_CORNER, keyframes.KF_SURF), leaf=0.4)
        assert 0 < len(gm) <= sum(len(clouds[i][0]) + len(clouds[i][1]) for i in sel)
    finally:
        store.close()
