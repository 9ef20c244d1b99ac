"""NDT registration (P2D / D2D) on the MI355X against the independent numpy reference tests/ndt_reference.py: the voxel maps, linearize / compute_error in
both modes over DIRECT1 / 7 / 27 / RADIUS(1.5) / RADIUS(2) at resolutions 0.5, 0.7, 1.0, 1.3, whole solves, every route a cloud can take, every refusal.

Voxel walls: no test excludes a term.  The clouds are drawn so that no transformed source element lies within 1e-4 * res of a voxel wall in the fp64
reference (ndt_reference.off_the_walls; asserted below on the CPU, the regenerated share asserted below 1 % -- measured with the reference alone:
0.3 % - 0.5 % of the points over four resolutions and two poses); test_points_on_walls puts points ON walls and asks only for the VGICP table's coordinate.
Measured on an MI355X (EXPERIMENTS.md "8a"): the figures each test prints."""
import ctypes as C
import os

import numpy as np
import pytest

import ndt_reference as nr

pytestmark = pytest.mark.gpu

CENTER = (100.0, -60.0, 2.0)
RES = [0.5, 0.7, 1.0, 1.3]
METHODS = [(nr.DIRECT1, 0.0), (nr.DIRECT7, 0.0), (nr.DIRECT27, 0.0), (nr.DIRECT_RADIUS, 1.5), (nr.DIRECT_RADIUS, 2.0)]


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import ndt, _lib
    return ndt, _lib


@pytest.fixture(scope="module")
def data():
    """target, source (a noisy part of the target seen from a pose within 0.3 m / 3 deg), that pose; every source point -- and, for D2D, every source
    voxel mean -- off the walls at identity and at the pose for every resolution under test"""
    rng = np.random.default_rng(9001)
    tgt = nr.scene(rng, 24000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)

    def make(k):
        p = nr.scene(rng, k).astype(np.float64)
        return (p @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (k, 3))).astype(np.float32)
    src, share = nr.off_the_walls(rng, make(8000), [np.eye(4), T], RES, make)
    assert share < 0.01, share
    # D2D's elements are the source voxels' means: a fixed function of the cloud, so a mean near a wall is moved by redrawing the whole cloud
    for attempt in range(50):
        ok = True
        for res in RES:
            m = nr.VoxelMap(src, res).mean
            for P in (np.eye(4), T):
                ok &= bool((nr.wall_distance(m @ P[:3, :3].T + P[:3, 3], res) >= 1e-4).all())
        if ok:
            break
        src, share = nr.off_the_walls(rng, make(8000), [np.eye(4), T], RES, make)
        assert share < 0.01, share
    assert ok and attempt < 5, attempt      # (means: ~2000 voxels x 3 axes x 2e-4 x 8 cases ~ one redraw in a few)
    for res in RES:
        for P in (np.eye(4), T):
            assert (nr.wall_distance(src.astype(np.float64) @ P[:3, :3].T + P[:3, 3], res) >= 1e-4).all()
    print("regenerated share of source points: %.4f, clouds redrawn for the means: %d" % (share, attempt))
    return dict(tgt=tgt, src=src, T=T)


def _product(mod, data, mode, method, radius, res):
    ndt, _ = mod
    r = ndt.NDTRegistration()
    r.setResolution(res)
    r.setDistanceMode(mode)
    r.setNeighborSearchMethod(method, radius)
    r.setInputTarget(data["tgt"])
    r.setInputSource(data["src"])
    return r


def _reference(data, mode, method, radius, res):
    ref = nr.NDT(res, mode, method, radius)
    ref.set_target(data["tgt"])
    ref.set_source(data["src"])
    return ref


_REF_MAPS = {}


def _ref_map(data, key, res, descending=False):
    k = (key, res, descending)
    if k not in _REF_MAPS:
        _REF_MAPS[k] = nr.VoxelMap(data[key], res, descending)
    return _REF_MAPS[k]


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("which", [0, 1])
def test_voxel_maps(mod, data, which, res):
    """Coordinates and counts equal as a set keyed by coordinate.  Means and covariances (before and after MIN_EIG): sum p p^T - mean (sum p)^T cancels
    (coordinates of 100 m against variances of 0.01 m^2), so the bound is measured, not fixed: the largest difference between the reference summing every
    voxel in ascending and in descending point index on these clouds, times 4 (two implementations that differ only in operation order sit inside a small
    multiple of the order-to-order spread; 4 leaves room for fused multiply-adds).  After MIN_EIG the eigen-solvers differ too (Jacobi against LAPACK):
    both are backward stable, each adds at most a few eps |C| -- 64 eps |C| is allowed on top."""
    r = _product(mod, data, nr.D2D, nr.DIRECT1, 0.0, res)
    got = r.voxels(which, raw=True)
    key = "tgt" if which == 0 else "src"
    up, down = _ref_map(data, key, res), _ref_map(data, key, res, True)
    order = np.lexsort((got["coords"][:, 2], got["coords"][:, 1], got["coords"][:, 0]))
    rorder = np.lexsort((up.coords[:, 2], up.coords[:, 1], up.coords[:, 0]))
    assert np.array_equal(got["coords"][order], up.coords[rorder]) and np.array_equal(got["n"][order], up.n[rorder])
    spread_m = np.abs(up.mean - down.mean).max()
    spread_c = np.abs(up.cov_raw - down.cov_raw).max()
    d_m = np.abs(got["mean"][order] - up.mean[rorder]).max()
    d_raw = np.abs(got["cov_raw"][order] - up.cov_raw[rorder]).max()
    d_cov = np.abs(got["cov"][order] - up.cov[rorder]).max()
    eig_slack = 64 * np.finfo(np.float64).eps * np.abs(up.cov).max()
    print("which %d res %.1f: %d voxels; spread mean %.3g cov %.3g; product mean %.3g raw cov %.3g clamped cov %.3g (eigen slack %.3g)"
          % (which, res, len(up.n), spread_m, spread_c, d_m, d_raw, d_cov, eig_slack))
    assert d_m <= 4 * spread_m and d_raw <= 4 * spread_c
    assert d_cov <= 4 * spread_c + eig_slack
    ev = np.linalg.eigvalsh(got["cov"])
    assert ev.min() >= 1e-3 - eig_slack


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("method,radius", METHODS)
@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_linearize_and_compute_error(mod, data, mode, method, radius, res):
    """number of terms equal; cost, H, b within 1e-5 relative (H and b: of their largest entry), at the pose and at identity; compute_error over the frozen
    list at a third pose"""
    r, ref = _product(mod, data, mode, method, radius, res), _reference(data, mode, method, radius, res)
    worst = 0.0
    for T in (data["T"], np.eye(4)):
        y, H, b = r.linearize(T)
        yr, Hr, br = ref.linearize(T)
        assert r.num_correspondences() == ref.num_terms() and ref.num_terms() > 50
        errs = (abs(y - yr) / abs(yr), np.abs(H - Hr).max() / np.abs(Hr).max(), np.abs(b - br).max() / np.abs(br).max())
        worst = max(worst, *errs)
        assert max(errs) <= 1e-5, errs
        assert np.array_equal(H, H.T)
        y2 = r.linearize(T, want_H=False)[0]
        assert y2 == y                                     # bit-identical from run to run
        T3 = nr.increment(np.array([0.002, -0.001, 0.003, 0.01, -0.02, 0.015]), T)[0]
        e, er = r.compute_error(T3), ref.compute_error(T3)
        assert abs(e - er) <= 1e-5 * abs(er)
        worst = max(worst, abs(e - er) / abs(er))
        assert r.compute_error(T) == pytest.approx(y, rel=1e-13)
    print("mode %d method %d r %.1f res %.1f: %d terms, worst relative difference %.3g" % (mode, method, radius, res, ref.num_terms(), worst))


@pytest.fixture(scope="module")
def shape_clouds():
    """a dense 6000-point room of 4 m (voxels of 0.5 m with far more than 6 points) and a lattice of 16500 points, ONE per voxel of 0.5 m (each
    0.02 m at most off its voxel's centre), nearest the room's fullest voxel first: the first n of them are n source points (P2D's elements) in n
    source voxels (D2D's).  The pose: 0.03 m along every axis, no rotation -- no point and no voxel mean comes near a wall."""
    rng = np.random.default_rng(9201)
    res = 0.5
    tgt = nr.scene(rng, 6000, half=2.0)
    vm = nr.VoxelMap(tgt, res)
    c0 = vm.coords[np.argmax(vm.n)]
    g = np.stack(np.meshgrid(np.arange(-13, 13), np.arange(-13, 13), np.arange(-12, 13), indexing="ij"), -1).reshape(-1, 3)
    g = g[np.argsort((g * g).sum(1), kind="stable")][:16500] + c0
    src = ((g + 1.0) * res + rng.uniform(-0.02, 0.02, g.shape)).astype(np.float32)   # voxel c holds [(c + 0.5) res, (c + 1.5) res): centre (c + 1) res
    T = np.eye(4)
    T[:3, 3] = 0.03
    assert len(np.unique(nr.voxel_coord(src.astype(np.float64), res), axis=0)) == 16500
    return dict(tgt=tgt, src=src, T=T, res=res)


@pytest.mark.parametrize("n", [1, 63, 257, 16500])
@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_block_sum_and_fold_shapes(mod, shape_clouds, mode, n):
    """the term kernel's block sums (with the term count) and the fold at 1 source element (one lane), 63 (a partial wave), 257 (a second workgroup of
    one lane) and 16500 (65 partial rows); the reference and the bound of test_linearize_and_compute_error"""
    d = dict(tgt=shape_clouds["tgt"], src=shape_clouds["src"][:n])
    r, ref = _product(mod, d, mode, nr.DIRECT7, 0.0, shape_clouds["res"]), _reference(d, mode, nr.DIRECT7, 0.0, shape_clouds["res"])
    if mode == nr.D2D:
        assert len(r.voxels(1)["n"]) == n
    for T in (shape_clouds["T"], np.eye(4)):
        y, H, b = r.linearize(T)
        yr, Hr, br = ref.linearize(T)
        assert r.num_correspondences() == ref.num_terms() and ref.num_terms() >= 1
        errs = (abs(y - yr) / abs(yr), np.abs(H - Hr).max() / np.abs(Hr).max(), np.abs(b - br).max() / np.abs(br).max())
        print("mode %d, %d elements: %d terms, relative differences %.3g %.3g %.3g" % ((mode, n, ref.num_terms()) + errs))
        assert max(errs) <= 1e-5, errs
        assert np.array_equal(H, H.T) and r.linearize(T, want_H=False)[0] == y
        assert r.compute_error(T) == pytest.approx(y, rel=1e-13)


def _pose_error(A, B):
    D = np.linalg.inv(A) @ B
    ang = np.arccos(np.clip(0.5 * (np.trace(D[:3, :3]) - 1), -1, 1))
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(ang)


@pytest.mark.parametrize("seed", [9101, 9102, 9103])
@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_align(mod, mode, seed):
    """T * cloud against cloud for a random SE(3) within 0.3 m / 3 deg with 1 cm sensor noise, from the identity guess: the pose within 1e-4 m / 1e-4 rad of
    the numpy reference running the same driver, iteration counts equal.  How close the minimum lies to the drawn pose is a property of the method (the source is
    a third of the target's points: its voxel means are not the target's), not of this implementation; asked of it is only that the solve ends nearer to
    the drawn pose than the identity guess it started from."""
    ndt, _ = mod
    rng = np.random.default_rng(seed)
    tgt = nr.scene(rng, 20000)
    T = nr.random_pose(rng, about=CENTER)
    Ti = np.linalg.inv(T)
    src = (tgt[::3].astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3] + rng.normal(0, 0.01, (len(tgt[::3]), 3))).astype(np.float32)
    r = ndt.NDTRegistration()
    r.setDistanceMode(mode)
    r.setInputTarget(tgt)
    r.setInputSource(src)
    got = r.align(np.eye(4)).astype(np.float64)
    ref = nr.NDT(1.0, mode, nr.DIRECT7)
    ref.set_target(tgt)
    ref.set_source(src)
    want, iters, conv, failed, Hfin = ref.align(np.eye(4))
    dt, da = _pose_error(got, want.astype(np.float32).astype(np.float64))
    gt, ga = _pose_error(got, T)
    print("mode %d seed %d: %d iterations (reference %d), to the reference %.3g m %.3g rad, to the drawn pose %.3g m %.3g rad" % (mode, seed, r.iterations(), iters, dt, da, gt, ga))
    assert dt <= 1e-4 and da <= 1e-4
    assert r.iterations() == iters and r.hasConverged() == conv and r.lmFailed() == failed
    assert np.abs(r.getFinalHessian() - Hfin).max() <= 1e-5 * np.abs(Hfin).max()
    g0, a0 = _pose_error(np.eye(4), T)
    assert gt < g0 and ga < a0


def _upload(L, h, a):
    d = C.c_void_p()
    assert L.rgc_device_alloc(h, a.nbytes, C.byref(d)) == 0
    assert L.rgc_upload(h, d, a.ctypes.data, a.nbytes) == 0
    return d


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_host_and_device_pointers_are_bit_identical(mod, data, mode):
    ndt, lib = mod
    a = _product(mod, data, mode, nr.DIRECT7, 0.0, 0.7)
    b = ndt.NDTRegistration()
    b.setResolution(0.7)
    b.setDistanceMode(mode)
    t4 = np.ascontiguousarray(np.concatenate([data["tgt"], np.ones((len(data["tgt"]), 1), np.float32)], 1))    # 16-byte stride on the device
    s8 = np.ascontiguousarray(np.concatenate([data["src"], np.zeros((len(data["src"]), 5), np.float32)], 1))   # 32-byte stride
    dt, ds = _upload(b._L, b._h, t4), _upload(b._L, b._h, s8)
    b._chk(b._L.rgc_ndt_set_target_device(b._h, dt, len(t4), 16))
    b._chk(b._L.rgc_ndt_set_source_device(b._h, ds, len(s8), 32))
    ya, Ha, ba = a.linearize(data["T"])
    yb, Hb, bb = b.linearize(data["T"])
    assert ya == yb and np.array_equal(Ha, Hb) and np.array_equal(ba, bb) and a.num_correspondences() == b.num_correspondences()
    assert np.array_equal(a.align(np.eye(4)), b.align(np.eye(4))) and a.iterations() == b.iterations()
    va, vb = a.voxels(0, raw=True), b.voxels(0, raw=True)
    for k in va:
        assert np.array_equal(va[k], vb[k]), k
    b._L.rgc_device_free(b._h, dt)
    b._L.rgc_device_free(b._h, ds)


def test_a_device_cloud_of_the_keyframe_store_as_target(mod, data):
    ndt, lib = mod
    from rgc_slam_amd.keyframes import KeyframeStore, KF_SURF
    r = ndt.NDTRegistration()
    store = KeyframeStore(r)
    tgt4 = np.concatenate([data["tgt"], np.zeros((len(data["tgt"]), 1), np.float32)], 1)
    half = len(tgt4) // 2
    store.push(0, np.zeros(6, np.float32), surf=tgt4[:half])
    store.push(1, np.zeros(6, np.float32), surf=tgt4[half:])
    dc = store.assemble([0, 1], (KF_SURF,), device=True)
    assert len(dc) == len(tgt4)
    r.setInputTarget(dc)                                   # stream-ordered: no synchronisation in between
    r.setInputSource(data["src"])
    host = _product(mod, data, nr.D2D, nr.DIRECT7, 0.0, 1.0)
    assert np.array_equal(dc.numpy()[:, :3], data["tgt"])  # (the identity pose leaves the points where they are)
    y, H, b = r.linearize(data["T"])
    yh, Hh, bh = host.linearize(data["T"])
    assert y == yh and np.array_equal(H, Hh) and np.array_equal(b, bh)
    dc.close()


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_swap_set_clear_set(mod, data, mode):
    ndt, lib = mod
    a = _product(mod, data, mode, nr.DIRECT7, 0.0, 1.0)
    a.linearize(np.eye(4))                                 # (both maps built before the swap in D2D)
    a.swapSourceAndTarget()
    b = ndt.NDTRegistration()
    b.setDistanceMode(mode)
    b.setInputTarget(data["src"])
    b.setInputSource(data["tgt"])
    Ti = np.linalg.inv(data["T"])
    ra, rb = a.linearize(Ti), b.linearize(Ti)
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert np.array_equal(a.align(np.eye(4)), b.align(np.eye(4)))
    # clear, then a solve is refused; set again, and the result is the first one's
    b.clearSource()
    with pytest.raises(ndt.RgcError) as e:
        b.align(np.eye(4))
    assert e.value.status == lib.ERR_NO_INPUT
    with pytest.raises(ndt.RgcError) as e:
        b.compute_error(np.eye(4))
    assert e.value.status == lib.ERR_NO_INPUT
    b.setInputSource(data["tgt"])
    r2 = b.linearize(Ti)
    assert r2[0] == rb[0] and np.array_equal(r2[1], rb[1])
    b.clearTarget()
    with pytest.raises(ndt.RgcError) as e:
        b.linearize(Ti)
    assert e.value.status == lib.ERR_NO_INPUT


def test_params_changed_between_linearize_and_compute_error(mod, data):
    """A new neighbour method or radius leaves the frozen terms in force (the precedent: rgc_set_params and the VGICP list); a new resolution or distance
    mode drops them."""
    ndt, lib = mod
    a = _product(mod, data, nr.P2D, nr.DIRECT7, 0.0, 1.0)
    y = a.linearize(data["T"])[0]
    n7 = a.num_correspondences()
    a.setNeighborSearchMethod(nr.DIRECT_RADIUS, 2.0)
    assert a.compute_error(data["T"]) == pytest.approx(y, rel=1e-13) and a.num_correspondences() == n7
    y33 = a.linearize(data["T"])[0]
    assert a.num_correspondences() > n7 and y33 > y
    a.setResolution(0.7)
    with pytest.raises(ndt.RgcError) as e:
        a.compute_error(data["T"])
    assert e.value.status == lib.ERR_INVALID
    a.linearize(data["T"])
    a.setDistanceMode(nr.D2D)
    with pytest.raises(ndt.RgcError) as e:
        a.compute_error(data["T"])
    assert e.value.status == lib.ERR_INVALID
    with pytest.raises(ndt.RgcError):
        a.num_correspondences()


def test_a_vgicp_solve_in_flight_is_left_alone(mod, data):
    ndt, lib = mod
    from rgc_slam_amd.registration import FastVGICP
    v = FastVGICP(0)
    v.setInputTarget(data["tgt"])
    v.setInputSource(data["src"])
    v.align(np.eye(4), want_output=False)
    want = v.getFinalTransformation().copy()
    want_it = v.nr_iterations
    v.setInputTarget(data["tgt"])
    v.setInputSource(data["src"])
    v.align_begin(np.eye(4))
    r = ndt.NDTRegistration(owner=v)                       # the same context
    r.setInputTarget(data["tgt"])
    r.setInputSource(data["src"])
    r.setDistanceMode(nr.P2D)
    y = r.linearize(data["T"])[0]
    r.align(np.eye(4))
    r.voxels(0)
    r.swapSourceAndTarget()
    r.clearSource()
    got = v.align_end()
    assert np.array_equal(got, want) and v.nr_iterations == want_it
    alone = _product(mod, data, nr.P2D, nr.DIRECT7, 0.0, 1.0)
    assert alone.linearize(data["T"])[0] == y
    r.close()
    v.close()


def test_refusals(mod, data, monkeypatch):
    ndt, lib = mod
    r = ndt.NDTRegistration()
    L, h = r._L, r._h
    before = r.getParams()

    def refused(**kw):
        p = lib.NdtParams(before["resolution"], before["distance_mode"], before["neighbor_method"], before["neighbor_radius"])
        for k, v in kw.items():
            setattr(p, k, v)
        return L.rgc_ndt_set_params(h, C.byref(p))
    for bad in (dict(resolution=0.0), dict(resolution=-1.0), dict(resolution=float("nan")), dict(resolution=float("inf")), dict(distance_mode=2), dict(distance_mode=-1),
                dict(neighbor_method=4), dict(neighbor_method=-1), dict(neighbor_method=3, neighbor_radius=-0.5), dict(neighbor_method=3, neighbor_radius=float("nan")),
                dict(neighbor_method=3, neighbor_radius=5.0), dict(neighbor_method=3, neighbor_radius=1e9)):
        assert refused(**bad) == lib.ERR_INVALID, bad
        assert r.getParams() == before
    assert refused(neighbor_method=3, neighbor_radius=4.8) == 0 and L.rgc_ndt_set_params(h, None) == lib.ERR_INVALID
    r.setNeighborSearchMethod(nr.DIRECT7)
    # the existing enum is what it was: DIRECT_RADIUS is NDT's only
    p = lib.default_params()
    p.neighbor_method = 3
    assert L.rgc_set_params(h, C.byref(p)) == lib.ERR_INVALID
    a = data["src"]
    T = (C.c_double * 16)(*np.eye(4).ravel())
    y = C.c_double(0)
    assert L.rgc_ndt_linearize(h, T, None, None, C.byref(y)) == lib.ERR_NO_INPUT          # a solve before both clouds are set
    g = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    assert L.rgc_ndt_align(h, g, None, None, None, None, None) == lib.ERR_NO_INPUT
    assert L.rgc_ndt_set_target(h, None, 10, 12) == lib.ERR_INVALID
    assert L.rgc_ndt_set_target(h, a.ctypes.data, 0, 12) == lib.ERR_TOO_FEW_POINTS and L.rgc_ndt_set_target(h, a.ctypes.data, -1, 12) == lib.ERR_INVALID
    assert L.rgc_ndt_set_target(h, a.ctypes.data, 10, 8) == lib.ERR_INVALID and L.rgc_ndt_set_target(h, a.ctypes.data, 10, 14) == lib.ERR_INVALID
    assert L.rgc_ndt_set_source(h, a.ctypes.data, (1 << 27) + 1, 12) == lib.ERR_INVALID
    assert L.rgc_ndt_linearize(h, T, None, None, C.byref(y)) == lib.ERR_NO_INPUT          # nothing was taken over
    r.setInputTarget(data["tgt"])
    r.setInputSource(a)
    Tn = (C.c_double * 16)(*np.eye(4).ravel())
    Tn[3] = float("nan")
    assert L.rgc_ndt_linearize(h, Tn, None, None, C.byref(y)) == lib.ERR_NONFINITE and L.rgc_ndt_linearize(h, None, None, None, C.byref(y)) == lib.ERR_INVALID
    gn = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    gn[7] = float("inf")
    assert L.rgc_ndt_align(h, gn, None, None, None, None, None) == lib.ERR_NONFINITE and L.rgc_ndt_align(h, None, None, None, None, None, None) == lib.ERR_INVALID
    assert L.rgc_ndt_compute_error(h, T, C.byref(y)) == lib.ERR_INVALID                   # no linearisation yet
    n = C.c_int(0)
    assert L.rgc_ndt_num_correspondences(h, C.byref(n)) == lib.ERR_INVALID
    assert L.rgc_ndt_get_voxels(h, 2, 0, None, None, None, None, C.byref(n)) == lib.ERR_INVALID and L.rgc_ndt_get_voxels(h, 0, -1, None, None, None, None, C.byref(n)) == lib.ERR_INVALID
    assert L.rgc_ndt_get_voxels(h, 0, 0, None, None, None, None, None) == lib.ERR_INVALID
    # a cloud with a non-finite point is refused by the call that builds its map, and a good cloud afterwards works
    bad = a.copy()
    bad[5, 1] = np.nan
    r.setInputSource(bad)
    r.setDistanceMode(nr.D2D)
    assert L.rgc_ndt_linearize(h, T, None, None, C.byref(y)) == lib.ERR_NONFINITE
    r.setInputSource(a)
    assert L.rgc_ndt_linearize(h, T, None, None, C.byref(y)) == 0 and y.value > 0
    # a grid beyond max_cells
    far = np.concatenate([data["tgt"], np.array([[1e6, 1e6, 1e5]], np.float32)])
    r.setInputTarget(far)
    assert L.rgc_ndt_linearize(h, T, None, None, C.byref(y)) == lib.ERR_GRID_TOO_LARGE
    r.close()
    # RGC_CHECK_POINTERS=1: a host pointer handed to a *_device entry is refused, not read
    monkeypatch.setenv("RGC_CHECK_POINTERS", "1")
    c = ndt.NDTRegistration()
    assert c._L.rgc_ndt_set_target_device(c._h, a.ctypes.data, len(a), 12) == lib.ERR_INVALID
    assert c._L.rgc_ndt_set_source_device(c._h, a.ctypes.data, len(a), 12) == lib.ERR_INVALID
    d = _upload(c._L, c._h, a)
    assert c._L.rgc_ndt_set_source_device(c._h, d, len(a) + 1, 12) == lib.ERR_INVALID      # a count beyond the allocation
    assert c._L.rgc_ndt_set_source_device(c._h, d, len(a), 12) == 0
    c._L.rgc_device_free(c._h, d)
    c.close()


@pytest.mark.parametrize("res", RES)
def test_points_on_walls(mod, res):
    """Points ON voxel walls (x = (k + 0.5) * res rounded to fp32, and its neighbours one ulp either side): the product's voxel coordinate is
    floor(x / res - 0.5) evaluated as the VGICP table evaluates it (fp32 point widened, fp64 division) -- the VGICP map of the same cloud, read through
    rgc_get_voxels, holds the same coordinates with the same counts."""
    ndt, lib = mod
    from rgc_slam_amd.registration import FastVGICP
    rng = np.random.default_rng(9201)
    k = rng.integers(-40, 40, (3000, 3))
    walls = ((k + 0.5) * res).astype(np.float32)
    pts = np.concatenate([walls, np.nextafter(walls, np.float32(1e9)), np.nextafter(walls, np.float32(-1e9))]).astype(np.float32)
    pts[:, 1:] += rng.uniform(0.1, 0.4, (len(pts), 2)).astype(np.float32) * np.float32(res) * (rng.integers(0, 2, (len(pts), 2)) > 0)
    r = ndt.NDTRegistration()
    r.setResolution(res)
    r.setInputTarget(pts)
    got = r.voxels(0)
    want = nr.voxel_coord(pts.astype(np.float64), res)
    uniq, cnt = np.unique(want, axis=0, return_counts=True)
    order = np.lexsort((got["coords"][:, 2], got["coords"][:, 1], got["coords"][:, 0]))
    assert np.array_equal(got["coords"][order], uniq) and np.array_equal(got["n"][order], cnt)
    v = FastVGICP(0)
    v.setResolution(res)
    v.setInputTarget(pts)
    vox = v.getVoxels()
    vc = np.asarray(vox["coords"] if isinstance(vox, dict) else vox[0]).reshape(-1, 3)
    assert np.array_equal(vc[np.lexsort((vc[:, 2], vc[:, 1], vc[:, 0]))], uniq)
    v.close()
    r.close()


def test_the_cpp_mirror_runs(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "rgc-slam_amd")
    exe = tmp_path / "test_ndt"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", os.path.join(root, "tests", "cpp", "test_ndt.cpp"), "-o", str(exe),
                           "-L", pkg, "-lrgc_hip", "-Wl,-rpath," + pkg])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0
