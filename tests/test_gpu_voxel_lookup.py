"""DIRECT1 / DIRECT7 / DIRECT27 and any voxel size on every GPU route, against tests/vgicp_reference.py (numpy).

The reference takes the covariances the GPU itself reports (getSourceCovariances / getTargetCovariances) as its input, so what is held
here is the voxel table, the look-ups with their offsets and H / b / cost; the covariances are held to tests/knn_reference.py at k = 20
at every resolution (the division branch of cell_coord and the k-NN walls at cell sizes that are not binary fractions):

  * the tuned route (PLANE, ADDITIVE) and the general route (RGC_FORCE_GENERAL=1, MIN_EIG, MULTIPLICATIVE) at resolutions
    {0.2, 0.3, 0.5, 0.75, 1.0, 1.7, 3.0}: voxels and correspondence counts exact, H / b / cost 1e-9;
  * align on the device-chained LM and on RGC_LM_IMPL=host with DIRECT7 / DIRECT27 against the oracle's solve; align_begin / align_end
    with a source of more than 32 768 points;
  * lazy (margin 0 is off; margins 1 and 2, margin 1 taking the miss path), re-framed (every reuse mode) and map-bound targets bit for
    bit against a plain target;
  * points on voxel walls (a checkerboard of occupied cells, so a point floored into the wrong cell changes the count), sources just
    outside the target's grid on each face, a target one cell thick, switching the method under frozen correspondences, a map 1e4 m out.

Cost on one MI355X: about 7 s, most of it the references on the CPU.
"""
import numpy as np
import pytest

import knn_reference as kr
import vgicp_reference as vr

pytestmark = pytest.mark.gpu

RES = [0.2, 0.3, 0.5, 0.75, 1.0, 1.7, 3.0]
METH = {"DIRECT27": 0, "DIRECT7": 1, "DIRECT1": 2}
CL = {}


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


@pytest.fixture(scope="module", autouse=True)
def clouds():
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(30000, seed=synth.SEED + 61)
    T_true = synth.se3(synth.rot_zyx(0.012, 0.002, -0.001), [0.11, 0.03, 0.002])
    CL.update(world=world, tgt=tgt, src=synth.make_scan_n(world, T_true, 8000, seed=synth.SEED + 61)["xyz"], T_true=T_true)
    CL["big_src"] = synth.make_scan_n(world, T_true, 40000, seed=synth.SEED + 62)["xyz"]
    CL["T_lin"] = synth.se3(synth.rot_zyx(0.015, -0.004, 0.003), [0.09, 0.05, -0.01])
    CL["T_err"] = synth.se3(synth.rot_zyx(0.0155, -0.0041, 0.0028), [0.094, 0.046, -0.012])
    for name in ("tgt", "src"):                 # the k-NN does not depend on the resolution: one reference per cloud
        idx, _ = kr.knn(CL[name], 20)
        S = kr.sample_covariances(CL[name], idx)
        CL[name + "_S"], CL[name + "_gap"] = S, kr.eigengap(S)
    yield
    CL.clear()


def _odo(reg_mod, res, method, mode=None, reg=None):
    v = reg_mod.odometer_vgicp(0)
    v.setResolution(res)
    v.setNeighborSearchMethod(METH[method])
    if reg is not None:
        v.setRegularizationMethod(reg)
    if mode is not None:
        v.setVoxelAccumulationMode(mode)
    return v


def _check_voxels(v, ref, what, mean_bar=1e-12):
    got = vr.in_cell_order(v.getVoxels())
    assert np.array_equal(got["coords"], ref["coords"]), f"{what}: voxel coordinates ({len(got['coords'])} vs {len(ref['coords'])})"
    assert np.array_equal(got["num"], ref["num"]), f"{what}: voxel counts"
    e = np.abs(got["mean"] - ref["mean"]).max(axis=1) / np.maximum(np.abs(ref["mean"]).max(axis=1), 1e-300)
    assert e.max(initial=0.0) <= mean_bar, f"{what}: voxel means {e.max():.2e}"
    assert vr.rel(got["cov"], ref["cov"]) <= 1e-9, f"{what}: voxel covariances {vr.rel(got['cov'], ref['cov']):.2e}"


def _check_linearize(v, tgt, src, res, method, mode, T_lin, T_err, what, table=None):
    """the GPU's voxels, linearisation and error against the reference on the GPU's own covariances; returns the reference's table"""
    if table is None:
        table = vr.voxel_table(tgt, v.getTargetCovariances(), res, mode)
        _check_voxels(v, table, what, 1e-9 if mode == "MULTIPLICATIVE" else 1e-12)
    sc = v.getSourceCovariances()
    cost, H, b = v.linearize(T_lin)
    rc, rH, rb, corr = vr.linearize(src, sc, table, T_lin, res, method)
    assert v.num_correspondences == len(corr["src"]), f"{what}: {v.num_correspondences} correspondences, reference {len(corr['src'])}"
    assert vr.rel(cost, rc) <= 1e-9 and vr.rel(H, rH) <= 1e-9 and vr.rel(b, rb) <= 1e-9, \
        f"{what}: cost {vr.rel(cost, rc):.1e} H {vr.rel(H, rH):.1e} b {vr.rel(b, rb):.1e}"
    e = v.compute_error(T_err)
    assert vr.rel(e, vr.compute_error(src, table, corr, T_err)) <= 1e-9, f"{what}: compute_error"
    return table, corr


def _check_knn(cov, name, what, method="PLANE"):
    ref = kr.regularize(CL[name + "_S"], method)
    ok = CL[name + "_gap"] >= kr.GAP_MIN if method == "PLANE" else np.ones(len(ref), bool)
    e = np.abs(cov - ref).reshape(len(ref), 9).max(axis=1)
    assert e[ok].max(initial=0.0) <= (1e-9 if method == "PLANE" else 1e-12 * np.abs(ref).max()), \
        f"{what}: {np.sum(e[ok] > 1e-9)} covariances off the k-NN reference, max {e[ok].max():.2e}"


@pytest.mark.parametrize("res", RES)
def test_tuned_route_every_method(reg_mod, res):
    tgt, src = CL["tgt"], CL["src"]
    v = _odo(reg_mod, res, "DIRECT1")
    v.setInputTarget(tgt); v.setInputSource(src)
    st = v.stats()
    print(f"tuned res={res}: cells {st['target_cells']} voxels {st['n_voxels']} deferred_target {st['deferred_target']} "
          f"deferred_source {st['deferred_source']}")
    _check_knn(v.getTargetCovariances(), "tgt", f"tuned res={res} map")
    _check_knn(v.getSourceCovariances(), "src", f"tuned res={res} scan")
    if res <= 0.3:       # small cells: the 3^3 block rarely holds the 20 nearest, the cooperative kernel answers the rest
        assert st["deferred_target"] > 0.1 * len(tgt), st
    table = None
    counts = {}
    for method in METH:
        v.setNeighborSearchMethod(METH[method])
        table, corr = _check_linearize(v, tgt, src, res, method, "ADDITIVE", CL["T_lin"], CL["T_err"], f"tuned res={res} {method}", table)
        counts[method] = len(corr["src"])
    assert counts["DIRECT1"] < counts["DIRECT7"] < counts["DIRECT27"], counts
    v.close()


@pytest.mark.parametrize("res", RES[1:])
def test_general_route_every_method(reg_mod, monkeypatch, res):
    tgt, src = CL["tgt"], CL["src"]
    monkeypatch.setenv("RGC_FORCE_GENERAL", "1")
    v = _odo(reg_mod, res, "DIRECT1", mode=reg_mod.FastVGICP.VOXEL_MULTIPLICATIVE, reg=reg_mod.FastVGICP.REG_MIN_EIG)
    monkeypatch.delenv("RGC_FORCE_GENERAL")
    v.setInputTarget(tgt); v.setInputSource(src)
    _check_knn(v.getTargetCovariances(), "tgt", f"general res={res} map", "MIN_EIG")
    table = None
    for method in METH:
        v.setNeighborSearchMethod(METH[method])
        table, _ = _check_linearize(v, tgt, src, res, method, "MULTIPLICATIVE", CL["T_lin"], CL["T_err"], f"general res={res} {method}", table)
    v.close()


def _rot_angle(Ra, Rb):
    R = Ra.astype(np.float64) @ Rb.astype(np.float64).T
    return float(np.arcsin(min(1.0, 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]))))


def _oracle_solve(orc, tgt, src, method, res=1.0):
    o = orc.Registration(k_correspondences=20, max_iterations=25, translation_eps=1e-6, num_threads=0, voxel_res=res, neighbor_method=METH[method])
    o.set_target(tgt); o.set_source(src)
    o.align(np.eye(4, dtype=np.float32))
    return o


def _against_oracle_solve(v, o, what):
    T, To = v.getFinalTransformation(), o.final_T
    dt, dth = float(np.abs(T[:3, 3] - To[:3, 3]).max()), _rot_angle(T[:3, :3], To[:3, :3])
    print(f"{what}: iterations {v.nr_iterations} / {o.iterations}, dt {dt:.1e} m, dtheta {dth:.1e} rad, "
          f"H {vr.rel(v.getFinalHessian(), o.final_H):.1e}")
    assert v.nr_iterations == o.iterations and v.hasConverged() == o.converged, what
    assert dt <= 1e-4 and dth <= 1e-4, what
    assert vr.rel(v.getFinalHessian(), o.final_H) <= 1e-6, what


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT27"])
@pytest.mark.parametrize("impl", ["device", "host"])
def test_align_both_lm_drivers(reg_mod, orc, monkeypatch, method, impl):
    if impl == "host":
        monkeypatch.setenv("RGC_LM_IMPL", "host")
    else:
        monkeypatch.delenv("RGC_LM_IMPL", raising=False)
    v = _odo(reg_mod, 1.0, method)
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["src"])
    v.align(np.eye(4, dtype=np.float32), want_output=False)
    _against_oracle_solve(v, _oracle_solve(orc, CL["tgt"], CL["src"], method), f"align {method} {impl}")
    v.close()


def test_align_begin_end_big_source(reg_mod, orc):
    """DIRECT27 with 40 000 source points: more than 128 partial rows, the second loop of block_fold_rows_pre"""
    v = _odo(reg_mod, 1.0, "DIRECT27")
    v.setInputTarget(CL["tgt"]); v.setInputSource(CL["big_src"])
    v.align_begin(np.eye(4, dtype=np.float32))
    v.align_end()
    _against_oracle_solve(v, _oracle_solve(orc, CL["tgt"], CL["big_src"], "DIRECT27"), "align_begin / end DIRECT27 40 k")
    v.close()


@pytest.mark.parametrize("method", ["DIRECT7", "DIRECT27"])
def test_lazy_reframed_and_map_bound_targets(reg_mod, method):
    import bench
    import rgc_slam_amd.synth as synth
    from rgc_slam_amd import local_map
    tgt, src = CL["tgt"], CL["src"]
    I4 = np.eye(4, dtype=np.float32)
    far = I4.copy(); far[:3, 3] = [0.9, -0.7, 0.2]                  # the solve moves across cells: look-ups leave the margin

    def solve(v, guess):
        v.align(guess, want_output=False)
        return v.getFinalTransformation(), v.nr_iterations, v.getFinalHessian()

    plain = _odo(reg_mod, 1.0, method)
    plain.setInputTarget(tgt); plain.setInputSource(src)
    want = {g: solve(plain, G) for g, G in (("near", I4), ("far", far))}
    for margin in (0, 1, 2):
        for g, G in (("near", I4), ("far", far)):
            lz = _odo(reg_mod, 1.0, method)
            lz.setLazyTarget(margin)
            lz.setInputTarget(tgt); lz.setInputSource(src)
            T, it, H = solve(lz, G)
            assert np.array_equal(T, want[g][0]) and it == want[g][1] and np.array_equal(H, want[g][2]), (method, margin, g)
            print(f"lazy {method} margin {margin} guess {g}: lazy_misses {lz.stats()['lazy_misses']}")
            if margin == 1 and g == "far":
                assert lz.stats()["lazy_misses"] >= 1, lz.stats()         # the miss path ran, and came out equal
            lz.close()
    # re-framed targets, every reuse mode, two frames
    n = len(tgt)
    a = np.zeros((n, 4), np.float32); a[:, :3] = tgt
    q, t = bench.world_to_body(synth.se3(synth.rot_zyx(0.3, 0.01, -0.02), [1.5, -1.0, 0.1]))
    ref = []
    for mode in (0, 1, 2):
        v = _odo(reg_mod, 1.0, method)
        v.setNeighbourReuse(mode)
        d_map, d_body = v.device_alloc(a.nbytes), v.device_alloc(a.nbytes)
        v.upload(d_map, a)
        for frame in range(2):
            v.setInputTargetReframed(d_map, n, 16, q, t, d_body)
            v.setInputSource(src)
            if not ref:
                # (a context's scan grid follows the crowding of its previous scan: the plain context sees the same scans in turn)
                body = v.download(d_body, (n, 4))[:, :3].copy()
                p2 = _odo(reg_mod, 1.0, method)
                p2.setInputTarget(body)
                for _ in range(2):
                    p2.setInputSource(src)
                    ref.append(solve(p2, I4))
                p2.close()
            T, it, H = solve(v, I4)
            assert np.array_equal(T, ref[frame][0]) and it == ref[frame][1] and np.array_equal(H, ref[frame][2]), (method, mode, frame)
        v.device_free(d_map); v.device_free(d_body)
        v.close()
    # a map-bound target: a one-keyframe map committed with a leaf filter, against the same points set plainly
    m_ctx = _odo(reg_mod, 1.0, method)
    m = local_map.RollingLocalMap(m_ctx)
    m.reset(np.zeros(3))
    m.insert(np.c_[tgt, np.zeros(n, np.float32)], np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    m.commit(0.1)
    m_ctx.setInputSource(src)
    T, it, H = solve(m_ctx, I4)
    p3 = _odo(reg_mod, 1.0, method)
    p3.setInputTarget(m.target()[:, :3].copy()); p3.setInputSource(src)
    Tp, itp, Hp = solve(p3, I4)
    assert np.array_equal(T, Tp) and it == itp and np.array_equal(H, Hp), method
    p3.close(); m_ctx.close(); plain.close()


def _checkerboard(res, rng, lo=-4, hi=4, per=6):
    """points inside every cell (cx + cy + cz) even of [lo, hi)^3, none in the others"""
    g = np.stack(np.meshgrid(*[np.arange(lo, hi)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[g.sum(axis=1) % 2 == 0]
    p = (g[:, None, :] + 0.5 + rng.uniform(0.15, 0.85, (len(g), per, 3))) * res
    return p.reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("res", [0.3, 0.75, 1.1])
def test_wall_points(reg_mod, res):
    """targets and sources on voxel walls; neighbouring cells alternate occupied / empty, so a point floored into the wrong cell
    changes the count and the cost.  At 1.1 the walls c = 7, 12, 22, 27 are binary fractions: x * (1 / res) floors a share of them
    into the other cell (tests/test_vgicp_reference.py::test_wall_points_are_sharp)"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(int(res * 100))
    cells = [-3, -1, 0, 2] + ([7, 12, 22, 27] if res == 1.1 else [])
    wv = vr.wall_values(res, cells)
    board = _checkerboard(res, rng)
    walls = np.stack([rng.choice(wv, 600), rng.choice(wv, 600), rng.choice(wv, 600)], axis=1).astype(np.float32)
    part = []                                                          # on a wall in x only, in x and y, inside the board in the others
    for a in (1, 2):
        w = walls.copy(); w[:, a:] = board[:600, a:]
        part.append(w)
    tgt = np.concatenate([board, walls] + part)
    R = Rotation.from_rotvec([0.3, -0.2, 0.5]).as_matrix()
    wp, poses, _, share = vr.wall_sources(res, R, np.array([-3, -2, -1, 0, 1, 2]), rng)
    src = np.concatenate([wp, board[::7], rng.choice(wv, (200, 3)).astype(np.float32)])
    for method in METH:
        v = _odo(reg_mod, res, method)
        v.setInputTarget(tgt); v.setInputSource(src)
        table, _ = _check_linearize(v, tgt, src, res, method, "ADDITIVE", np.eye(4), CL["T_err"], f"walls res={res} {method} identity")
        for j in range(len(poses)):
            _check_linearize(v, tgt, src, res, method, "ADDITIVE", poses[j], poses[j], f"walls res={res} {method} pose {j}", table)
        v.close()
    print(f"walls res={res}: {len(tgt)} target points, {len(table['num'])} voxels; pose-product share {share:.2f}")


def test_sources_outside_each_face_and_a_thin_target(reg_mod):
    """DIRECT27: source points half a cell outside the target's grid on each of the six faces reach occupied voxels only through an
    offset; and a target one cell thick in z (dim[2] == 1)"""
    rng = np.random.default_rng(8)
    res = 0.75
    tgt = (rng.uniform(0.0, 6.0, (4000, 3)) * res).astype(np.float32) + np.float32(0.5 * res)
    lo, hi = tgt.min(axis=0), tgt.max(axis=0)
    out = []
    for a in range(3):
        for side, edge in ((-1, lo[a]), (1, hi[a])):
            p = rng.uniform(lo, hi, (100, 3))
            p[:, a] = edge + side * 0.5 * res
            out.append(p)
    src = np.concatenate(out).astype(np.float32)
    thin = tgt.copy(); thin[:, 2] = np.float32(0.9 * res)            # every point in cell z = 0
    for name, t in (("box", tgt), ("thin", thin)):
        for method in METH:
            v = _odo(reg_mod, res, method)
            v.setInputTarget(t); v.setInputSource(src)
            _, corr = _check_linearize(v, t, src, res, method, "ADDITIVE", np.eye(4), CL["T_err"], f"{name} {method}")
            if method == "DIRECT1" and name == "box":
                assert len(corr["src"]) == 0
            if method == "DIRECT27":
                assert len(corr["src"]) > 0
            v.close()


def test_switching_the_method(reg_mod):
    """compute_error uses the correspondences frozen by the last linearisation whatever the method is now (the reference keeps
    voxel_correspondences_); a solve after a switch re-sizes the buffers and equals a fresh context's, bit for bit.  Regression:
    rgc_set_params dropped the correspondences on every call, so compute_error after setNeighborSearchMethod was refused."""
    tgt, src, res = CL["tgt"], CL["src"], 0.75
    v = _odo(reg_mod, res, "DIRECT27")
    v.setInputTarget(tgt); v.setInputSource(src)
    table = vr.voxel_table(tgt, v.getTargetCovariances(), res, "ADDITIVE")
    sc = v.getSourceCovariances()
    for first, then in (("DIRECT27", "DIRECT1"), ("DIRECT1", "DIRECT7"), ("DIRECT7", "DIRECT27")):
        v.setNeighborSearchMethod(METH[first])
        v.linearize(CL["T_lin"])
        v.setNeighborSearchMethod(METH[then])
        _, _, _, corr = vr.linearize(src, sc, table, CL["T_lin"], res, first)
        assert vr.rel(v.compute_error(CL["T_err"]), vr.compute_error(src, table, corr, CL["T_err"])) <= 1e-9, (first, then)
    I4 = np.eye(4, dtype=np.float32)
    for m1, m2 in (("DIRECT1", "DIRECT27"), ("DIRECT27", "DIRECT7"), ("DIRECT7", "DIRECT1")):
        v.setNeighborSearchMethod(METH[m1])
        v.align(I4, want_output=False)
        v.setNeighborSearchMethod(METH[m2])
        v.align(I4, want_output=False)
        w = _odo(reg_mod, res, m2)
        w.setInputTarget(tgt); w.setInputSource(src)
        w.align(I4, want_output=False)
        assert np.array_equal(v.getFinalTransformation(), w.getFinalTransformation()) and v.nr_iterations == w.nr_iterations, (m1, m2)
        assert np.array_equal(v.getFinalHessian(), w.getFinalHessian()), (m1, m2)
        w.close()
    v.close()


def test_far_offset_map(reg_mod):
    """the map and scan 1e4 m from the origin at res 0.75 with DIRECT7"""
    off = np.float32([1.0e4, -1.0e4, 3.0e3])
    tgt, src = CL["tgt"] + off, CL["src"] + off
    S = off.astype(np.float64)
    Tl, Te = CL["T_lin"].copy(), CL["T_err"].copy()
    Tl[:3, 3] += S - Tl[:3, :3] @ S
    Te[:3, 3] += S - Te[:3, :3] @ S
    v = _odo(reg_mod, 0.75, "DIRECT7")
    v.setInputTarget(tgt); v.setInputSource(src)
    _check_linearize(v, tgt, src, 0.75, "DIRECT7", "ADDITIVE", Tl, Te, "far DIRECT7")
    v.close()
