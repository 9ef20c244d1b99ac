"""Exact k-NN and covariances on the GPU over the whole k range the API accepts (2..32) and on every kernel that can answer a query.

The device code splits k three ways, each a different instance: k == 20 (the reference's setting, the kExact instances, the only ones with
seeds and neighbour lists), k < 20 (the 20-slot instances with the general-k branches) and k > 20 (the 32-slot instances, whose k == KC
branches only k = 32 takes); the general route (k_knn_cov6, k_voxel_*_coop) has its own <20> / <32> split.  At every k of K below, on
fresh contexts, each route is checked against the CPU oracle and against tests/knn_reference.py (numpy / scipy), which
tests/test_knn_reference.py holds the oracle equal to at every k:

  * a dense 60 k-point map as the target (the one-lane bulk search) and a raw 30 k-point scan as the source (the four-lane split
    search, its 3^3 block and then the 5^3 one): covariances, voxel table, linearisation (k >= 3), the pose of a solve (k >= 5);
  * a sparse map of three leaf-filtered sweeps (the wide block, k_knn_sp_wide);
  * an anisotropic lattice with exact duplicates (ties at the k-th key: the cooperative kernel, on both clouds);
  * clouds of n = k, k + 1, 64 and 65 points;
  * k + 5 copies of the origin and an exactly collinear pole inside a map (rank 0 / rank 1: the Jacobi fallback picks the normal);
  * the general route (RGC_FORCE_GENERAL=1, REG_NONE): the raw covariance against the reference's, the direct check of the neighbour set;
  * re-framed targets under every reuse mode and the lazy target, bit for bit against a plain setInputTarget of the same points.

Cost on one MI355X: about 15 s (measured once, inside the whole -m gpu run), most of it the oracle and the reference on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_reference as kr

pytestmark = pytest.mark.gpu

K = [2, 3, 4, 5, 8, 11, 16, 19, 20, 21, 24, 26, 31, 32]
POLE_XY = (2.375, -1.625)


@pytest.fixture(scope="module")
def reg_mod():
    from rgc_slam_amd import registration
    return registration


def _rot_angle(Ra, Rb):
    R = Ra.astype(np.float64) @ Rb.astype(np.float64).T
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arcsin(min(1.0, np.linalg.norm(w))))


def _odo(reg_mod, k):
    v = reg_mod.odometer_vgicp(0)
    v.setCorrespondenceRandomness(k)
    return v


def _oracle(orc, tgt, src, k):
    o = orc.Registration(k_correspondences=k, max_iterations=25, translation_eps=1e-6, num_threads=0)
    o.set_target(tgt); o.set_source(src); o.prepare()
    return o


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    """(PLANE covariance, eigengap, raw covariance) of cloud `name` at k, from the numpy / scipy reference"""
    pts = CLOUDS[name]
    idx, _ = kr.knn(pts, k)
    S = kr.sample_covariances(pts, idx)
    return kr.regularize(S, "PLANE"), kr.eigengap(S), S


CLOUDS = {}


@pytest.fixture(scope="module", autouse=True)
def clouds(orc):
    import rgc_slam_amd.synth as synth
    world, tgt = synth.make_world_and_map(60000, seed=synth.SEED + 41)
    T_true = synth.se3(synth.rot_zyx(0.012, 0.002, -0.001), [0.11, 0.03, 0.002])
    CLOUDS["dense"], CLOUDS["scan"], CLOUDS["T_true"] = tgt, synth.make_scan_n(world, T_true, 30000, seed=synth.SEED + 41)["xyz"], T_true
    # the sparse map of test_sparse_map_takes_the_wide_block: three leaf-filtered 16-beam sweeps
    w2 = synth.make_world(half_extent=45.0, seed=synth.SEED)
    poses = synth.make_trajectory(5, seed=synth.SEED)
    sweeps = [synth.make_scan(w2, poses[i], n_az=900, seed=synth.SEED + 70 + i)["xyz"] for i in range(4)]
    to_world = lambda xyz, T: (xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    cat = np.concatenate([np.c_[to_world(sweeps[i], poses[i]), np.zeros(len(sweeps[i]), np.float32)] for i in range(3)])
    CLOUDS["sparse"] = orc.voxelgrid_filter(cat, 0.3)[:, :3].copy()
    CLOUDS["sparse_src"] = orc.voxelgrid_filter(np.c_[sweeps[3], np.zeros(len(sweeps[3]), np.float32)], 0.2)[:, :3].copy()
    CLOUDS["sparse_T"] = poses[3]
    rng = np.random.default_rng(41)
    g = np.stack(np.meshgrid(np.arange(14), np.arange(14), np.arange(5), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    g = g * np.float32((0.25, 0.27, 0.31))
    lat = np.concatenate([g, g[rng.choice(len(g), 150, replace=False)]])
    CLOUDS["lattice"] = lat[rng.permutation(len(lat))] + np.float32([3.0, -2.0, 0.5])
    CLOUDS["lattice_src"] = CLOUDS["lattice"][:400].copy()
    # a 20 k slice of the map around the origin with a pole in a 2 m clearing; the k + 5 copies of the origin are added per k
    base = tgt[::3] - tgt.mean(axis=0).astype(np.float32)
    clear = np.hypot(base[:, 0] - POLE_XY[0], base[:, 1] - POLE_XY[1]) > 2.0
    pole = np.stack([np.full(60, POLE_XY[0]), np.full(60, POLE_XY[1]), np.linspace(0.0, 3.0, 60)], axis=1).astype(np.float32)
    CLOUDS["degenerate_base"] = np.concatenate([base[clear], pole])
    yield
    CLOUDS.clear()
    _ref.cache_clear()


def _cov_rows_above(got, exp, tol=1e-9):
    return int(np.sum(np.abs(got - exp).reshape(len(got), 9).max(axis=1, initial=0.0) > tol))


def _against_oracle(got, exp, name, k, what):
    """PLANE covariances against the oracle's: no row above 1e-9 where the reference's eigengap defines the normal.  Where it does not (a
    neighbourhood of rank 1: every row at k = 2, the odd collinear triple at k = 3) any unit vector of the null space is the normal, the
    Jacobi sweeps of the two sides pick different ones, and the row must instead be I - 0.999 n n^T with n in that null space.  Returns
    the number of such rows."""
    _, gap, S = _ref(name, k)
    ok = gap >= kr.GAP_MIN
    assert _cov_rows_above(got[ok], exp[ok]) == 0, f"{what} k={k}: {_cov_rows_above(got[ok], exp[ok])} covariances off the oracle"
    if (~ok).any():
        w, U = np.linalg.eigh(got[~ok])
        assert np.abs(w - [1e-3, 1.0, 1.0]).max() <= 1e-12, f"{what} k={k}: not I - 0.999 n n^T"
        n = U[:, :, 0]
        tr = np.trace(S[~ok], axis1=1, axis2=2)
        assert np.all(np.einsum("ni,nij,nj->n", n, S[~ok], n) <= 2 * kr.GAP_MIN * tr), f"{what} k={k}: normal outside the null space"
    return int(np.sum(~ok))


def _against_reference(got, name, k, what):
    """PLANE covariances against the reference on rows whose eigengap defines the normal; returns the number of rows skipped"""
    plane, gap, _ = _ref(name, k)
    ok = gap >= kr.GAP_MIN
    e = np.abs(got - plane).reshape(len(got), -1).max(axis=1)
    assert e[ok].max(initial=0.0) <= 1e-9, f"{what} k={k}: {np.sum(e[ok] > 1e-9)} rows off the reference, max {e[ok].max():.2e}"
    return int(np.sum(~ok))


def _voxels_equal_oracle(v, o, what, k):
    vm, om = v.getVoxels(), o.voxelmap()
    assert np.array_equal(vm["coords"], om["coords"]) and np.array_equal(vm["num"], om["num"]), f"{what} k={k}: voxel table"
    assert np.abs(vm["mean"] - om["mean"]).max() <= 1e-9, f"{what} k={k}: voxel means"
    if k >= 3:      # (k = 2: every point's normal is any unit vector of a plane, the voxels sum such choices)
        assert np.abs(vm["cov"] - om["cov"]).max() <= 1e-9, f"{what} k={k}: voxel covariances"


@pytest.mark.parametrize("k", K)
def test_dense_map_and_raw_scan(reg_mod, orc, k):
    """the one-lane bulk search (the map) and the four-lane split search (the scan) against the oracle and the reference"""
    tgt, src, T_true = CLOUDS["dense"], CLOUDS["scan"], CLOUDS["T_true"]
    v = _odo(reg_mod, k)
    v.setInputTarget(tgt); v.setInputSource(src)
    st = v.stats()
    print(f"dense k={k}: n_target {st['n_target']} cells {st['target_cells']} deferred_target {st['deferred_target']} "
          f"deferred_source {st['deferred_source']} searched_target {st['searched_target']}")
    assert st["n_target"] >= 0.25 * st["target_cells"]                  # dense: not the wide block
    o = _oracle(orc, tgt, src, k)
    ct, cs = v.getTargetCovariances(), v.getSourceCovariances()
    _against_oracle(ct, o.target_cov(len(tgt)), "dense", k, "map")
    _against_oracle(cs, o.source_cov(len(src)), "scan", k, "scan")
    skipped = (_against_reference(ct, "dense", k, "map"), _against_reference(cs, "scan", k, "scan"))
    print(f"dense k={k}: rows skipped for PLANE against the reference (map, scan): {skipped}")
    _voxels_equal_oracle(v, o, "dense", k)
    guess = np.asarray(T_true, np.float64).copy(); guess[:3, 3] += [0.03, -0.02, 0.01]
    if k >= 3:
        cost, H, b = v.linearize(guess)
        ocost, oH, ob = o.linearize(guess)
        assert abs(cost - ocost) <= 1e-9 * abs(ocost), (k, cost, ocost)
        assert np.abs(H - oH).max() <= 1e-9 * np.abs(oH).max() and np.abs(b - ob).max() <= 1e-9 * np.abs(ob).max(), k
    I4 = np.eye(4, dtype=np.float32)
    v.align(I4, want_output=False)
    T = v.getFinalTransformation()
    if k >= 5:
        To = o.align(I4)
        assert np.abs(T[:3, 3] - To[:3, 3]).max() <= 1e-4 and _rot_angle(T[:3, :3], To[:3, :3]) <= 1e-4, k
    # the lazy target: the full build's pose and covariances, bit for bit
    lz = _odo(reg_mod, k)
    lz.setLazyTarget(2)
    lz.setInputTarget(tgt); lz.setInputSource(src)
    lz.align(I4, want_output=False)
    assert np.array_equal(lz.getFinalTransformation(), T) and lz.nr_iterations == v.nr_iterations, k
    assert np.array_equal(lz.getTargetCovariances(), ct), k
    lz.close(); v.close()


@pytest.mark.parametrize("k", K)
def test_sparse_map_wide_block(reg_mod, orc, k):
    tgt, src = CLOUDS["sparse"], CLOUDS["sparse_src"]
    v = _odo(reg_mod, k)
    v.setInputTarget(tgt); v.setInputSource(src)
    st = v.stats()
    print(f"sparse k={k}: n_target {st['n_target']} cells {st['target_cells']} deferred_target {st['deferred_target']} "
          f"deferred_source {st['deferred_source']}")
    assert st["n_target"] < 0.25 * st["target_cells"], st                # the wide block is the map's route
    # ... and it settled most queries itself (recorded on this map: 0 at k <= 3, 9 % at k = 20, 21 % at k = 32 -- the 5^3 block holds
    # fewer of the 32 nearest -- where the 3^3 block of the dense-map kernel leaves ~85 % to the cooperative kernel)
    assert st["deferred_target"] < 0.25 * st["n_target"], st
    o = _oracle(orc, tgt, src, k)
    ct = v.getTargetCovariances()
    _against_oracle(ct, o.target_cov(len(tgt)), "sparse", k, "sparse map")
    _against_oracle(v.getSourceCovariances(), o.source_cov(len(src)), "sparse_src", k, "sparse map's source")
    print(f"sparse k={k}: rows skipped for PLANE: {_against_reference(ct, 'sparse', k, 'sparse map')}")
    _voxels_equal_oracle(v, o, "sparse", k)
    v.close()


@pytest.mark.parametrize("k", K)
def test_lattice_with_duplicates_cooperative_kernel(reg_mod, orc, k):
    tgt, src = CLOUDS["lattice"], CLOUDS["lattice_src"]
    v = _odo(reg_mod, k)
    v.setInputTarget(tgt); v.setInputSource(src)
    st = v.stats()
    print(f"lattice k={k}: deferred_target {st['deferred_target']} deferred_source {st['deferred_source']}")
    assert st["deferred_target"] > 0 and st["deferred_source"] > 0, st  # the cooperative kernel ran on both clouds
    o = _oracle(orc, tgt, src, k)
    ct, cs = v.getTargetCovariances(), v.getSourceCovariances()
    _against_oracle(ct, o.target_cov(len(tgt)), "lattice", k, "lattice")
    _against_oracle(cs, o.source_cov(len(src)), "lattice_src", k, "lattice as source")
    print(f"lattice k={k}: rows skipped for PLANE: {_against_reference(ct, 'lattice', k, 'lattice')}")
    _voxels_equal_oracle(v, o, "lattice", k)
    v.close()


@pytest.mark.parametrize("k", K)
def test_tiny_clouds(reg_mod, orc, k):
    """n = k: every row is the whole cloud -- the same covariance in every row (to the rounding of the moments, which the kernels take
    about each query point)"""
    rng = np.random.default_rng(500 + k)
    for n in (k, k + 1, 64, 65):
        pts = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
        name = f"tiny{n}_{k}"
        CLOUDS[name] = pts
        v = _odo(reg_mod, k)
        v.setInputTarget(pts); v.setInputSource(pts)
        ct, cs = v.getTargetCovariances(), v.getSourceCovariances()
        o = _oracle(orc, pts, pts, k)
        _against_oracle(ct, o.target_cov(n), name, k, f"tiny n={n}")
        _against_oracle(cs, o.source_cov(n), name, k, f"tiny n={n} as source")
        _against_reference(ct, name, k, f"tiny n={n}")
        _against_reference(cs, name, k, f"tiny n={n} as source")
        if n == k and _ref(name, k)[1][0] >= kr.GAP_MIN:
            assert np.abs(ct - ct[0]).max() <= 1e-9 and np.abs(cs - ct[0]).max() <= 1e-9, (k, n)
        _voxels_equal_oracle(v, o, f"tiny n={n}", k)
        v.close()


@pytest.mark.parametrize("k", K)
def test_degenerate_neighbourhoods(reg_mod, orc, k):
    """rank 0 (k + 5 copies of the origin) and rank 1 (an exactly collinear pole): the normal is the Jacobi fallback's choice, the oracle's
    bit for bit; the covariance is I - 0.999 n n^T (the oracle's U diag(1, 1, 1e-3) U^T to the last bit of 1e-3).  Regression, every k,
    the tuned route (map and scan searches, min_eigenvector): the pole's moments are exactly diag(0, 0, s), and the fallback took the
    LAST of the two zero eigenvalues' columns -- normal (0, 1, 0) -- where the oracle's selection sort, like Eigen's JacobiSVD, ends on
    column 0 -- normal (1, 0, 0)."""
    rng = np.random.default_rng(900 + k)
    pts = np.concatenate([CLOUDS["degenerate_base"], np.zeros((k + 5, 3), np.float32)])
    pts = pts[rng.permutation(len(pts))]
    CLOUDS[f"degenerate{k}"] = pts
    v = _odo(reg_mod, k)
    v.setInputTarget(pts); v.setInputSource(pts)
    ct, nt = v.getTargetCovariances(), v.getTargetNormals()
    cs, ns = v.getSourceCovariances(), v.getSourceNormals()
    ocov, onrm = orc.covariances(pts, k=k)
    idx, _ = kr.knn(pts, k)
    zero = np.all(pts[idx] == 0.0, axis=(1, 2))
    line = np.all((pts[idx][:, :, 0] == np.float32(POLE_XY[0])) & (pts[idx][:, :, 1] == np.float32(POLE_XY[1])), axis=1)
    assert zero.sum() == k + 5 and line.sum() == 60, (k, zero.sum(), line.sum())
    for c, nn, what in ((ct, nt, "target"), (cs, ns, "source")):
        assert np.array_equal(nn[zero], onrm[zero]), f"k={k} {what}: rank-0 normals {nn[zero][:2]} vs oracle {onrm[zero][:2]}"
        assert np.abs(c[zero] - np.diag([1.0, 1.0, 1e-3])).max() <= 1e-15, f"k={k} {what}: rank 0"
        assert np.array_equal(nn[line], onrm[line]), f"k={k} {what}: pole normals {nn[line][:2]} vs oracle {onrm[line][:2]}"
        assert np.all(nn[line][:, 2] == 0.0) and np.all(np.abs(np.linalg.norm(nn[line], axis=1) - 1.0) <= 1e-15), k
        assert np.abs(c[zero | line] - ocov[zero | line]).max() <= 1e-15, k
        _against_oracle(c, ocov, f"degenerate{k}", k, f"degenerate {what}")
        _against_reference(c, f"degenerate{k}", k, f"degenerate {what}")
    v.close()


@pytest.mark.parametrize("k", K)
def test_general_route_raw_covariances(reg_mod, monkeypatch, k):
    """RGC_FORCE_GENERAL=1 and REG_NONE: k_knn_cov6 hands out the sample covariance itself -- to 1e-12 of the reference's, row by row, so
    the neighbour set of every query is the reference's"""
    monkeypatch.setenv("RGC_FORCE_GENERAL", "1")
    g = _odo(reg_mod, k)
    monkeypatch.delenv("RGC_FORCE_GENERAL")
    g.setRegularizationMethod(g.REG_NONE)
    for tname, sname in (("dense", "scan"), ("lattice", "lattice_src")):
        g.setInputTarget(CLOUDS[tname]); g.setInputSource(CLOUDS[sname])
        for got, name in ((g.getTargetCovariances(), tname), (g.getSourceCovariances(), sname)):
            e = kr.row_rel_err(got, _ref(name, k)[2])
            assert e.max() <= 1e-12, f"general route k={k} {name}: {np.sum(e > 1e-12)} rows off the reference, max {e.max():.2e}"
    g.close()


@pytest.mark.parametrize("k", K)
def test_reframed_target_every_reuse_mode(reg_mod, k):
    """setInputTargetReframed under reuse modes 0 / 1 / 2, two frames on an unchanged map: the covariances and voxels of a plain
    setInputTarget of the re-framed points, bit for bit.  Seeds and lists exist at k = 20 only: at any other k every point is searched."""
    import bench
    import rgc_slam_amd.synth as synth
    tgt = CLOUDS["dense"]
    n = len(tgt)
    a = np.zeros((n, 4), np.float32); a[:, :3] = tgt
    q, t = bench.world_to_body(synth.se3(synth.rot_zyx(0.4, 0.01, -0.02), [2.0, -1.0, 0.1]))
    plain = _odo(reg_mod, k)
    for mode in (0, 1, 2):
        v = _odo(reg_mod, k)
        v.setNeighbourReuse(mode)
        d_map, d_body = v.device_alloc(a.nbytes), v.device_alloc(a.nbytes)
        v.upload(d_map, a)
        searched = []
        for frame in range(2):
            v.setInputTargetReframed(d_map, n, 16, q, t, d_body)
            c = v.getTargetCovariances()
            searched.append(v.stats()["searched_target"])
            if mode == 0 and frame == 0:
                plain.setInputTarget(v.download(d_body, (n, 4))[:, :3].copy())
                cp, xp = plain.getTargetCovariances(), plain.getVoxels()
            assert np.array_equal(c, cp), (k, mode, frame)
            xv = v.getVoxels()
            assert all(np.array_equal(xv[key], xp[key]) for key in ("coords", "num", "mean", "cov")), (k, mode, frame)
        print(f"reframed k={k} mode {mode}: searched_target per frame {searched} of {n}")
        if k != 20:
            assert searched == [n, n], (k, mode, searched)
        elif mode == 2:
            assert searched[1] < n, searched                            # (k = 20: the lists of the unchanged map answer most queries)
        v.device_free(d_map); v.device_free(d_body)
        v.close()
    plain.close()


def _params(v):
    from rgc_slam_amd import _lib
    p = _lib.Params()
    assert v._L.rgc_get_params(v._h, C.byref(p)) == 0
    return p


def test_k_outside_2_to_32_is_refused(reg_mod):
    """k = 1 and k = 33: RGC_ERR_INVALID, the parameters and the prepared clouds as they were"""
    from rgc_slam_amd import _lib
    tgt, src = CLOUDS["lattice"], CLOUDS["lattice_src"]
    v = _odo(reg_mod, 7)
    v.setInputTarget(tgt); v.setInputSource(src)
    before, c0 = _params(v), v.getTargetCovariances()
    for bad in (1, 33, 0, -1):
        p = _lib.Params.from_buffer_copy(before)
        p.k_correspondences = bad
        assert v._L.rgc_set_params(v._h, C.byref(p)) == _lib.ERR_INVALID, bad
        assert bytes(_params(v)) == bytes(before), bad
    assert np.array_equal(v.getTargetCovariances(), c0)
    for good in (2, 32):
        p = _lib.Params.from_buffer_copy(before)
        p.k_correspondences = good
        assert v._L.rgc_set_params(v._h, C.byref(p)) == 0, good
    v.close()


@pytest.mark.parametrize("k", [2, 32])
def test_k_minus_one_points_are_too_few(reg_mod, k):
    from rgc_slam_amd import _lib
    pts = np.random.default_rng(k).uniform(-1.0, 1.0, (k, 3)).astype(np.float32)
    v = _odo(reg_mod, k)
    for setter in (v.setInputTarget, v.setInputSource):
        with pytest.raises(reg_mod.RgcError) as e:
            setter(pts[:k - 1])
        assert e.value.status == _lib.ERR_TOO_FEW_POINTS
        setter(pts)                                                          # exactly k: accepted
    v.close()


def test_changing_k_after_the_clouds_are_set(reg_mod):
    """setCorrespondenceRandomness with both clouds set re-prepares them (rgc_set_params' redo path): the covariances and voxels of a
    fresh context with that k, bit for bit -- from 20 (the kExact instances) to 7, from 7 to 32 and from 32 back to 20"""
    tgt, src = CLOUDS["dense"][::2].copy(), CLOUDS["scan"]
    v = _odo(reg_mod, 20)
    v.setInputTarget(tgt); v.setInputSource(src)
    for k in (7, 32, 20):
        v.setCorrespondenceRandomness(k)
        w = _odo(reg_mod, k)
        w.setInputTarget(tgt); w.setInputSource(src)
        assert np.array_equal(v.getTargetCovariances(), w.getTargetCovariances()), k
        assert np.array_equal(v.getSourceCovariances(), w.getSourceCovariances()), k
        xv, xw = v.getVoxels(), w.getVoxels()
        assert all(np.array_equal(xv[key], xw[key]) for key in ("coords", "num", "mean", "cov")), k
        w.close()
    v.close()
