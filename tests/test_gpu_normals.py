"""Surface normal estimation (rgc_normal_*, features.NormalEstimation, Preprocessor.normalEstimation) on the MI355X against the independent numpy reference
tests/normal_reference.py, on the designed cases of tests/normal_cases.py (tests/test_normal_reference.py shows on the CPU what each case contains).

Equality where the header promises it: the member counts, n_valid, the NaN rows, the sign wherever the reference's dot product exceeds its bound, and the
bytes of the k route across cell sizes, pointers, strides and runs.  Every tolerance is the reference's, derived there from the sums of absolute terms
(normal_reference's docstring): the covariance and the centroid entry by entry, the eigenvalue through curvature * trace (Weyl, plus one fp32 ulp), every valid
normal's length (two fp32 ulps) and residual |S n - lambda n| (no gap needed: eight times the eigenvalue bound for the solver, plus the fp32 roundings of n
and of the curvature, 2^-23 (|S|_F + lambda)), every decided normal within bound_n of the reference's.  Each comparison prints its largest error / tolerance.
A reference is computed once per (case, run) and shared (normal_cases.ref)."""
import ctypes as C

import numpy as np
import pytest

import knn_reference as kr
import normal_cases as nc
import search_reference as sr

pytestmark = pytest.mark.gpu

CASES = nc.cases()
RUNS = [(name, i) for name in CASES for i in range(len(CASES[name]["runs"]))]


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, features
    return features, _lib


@pytest.fixture(scope="module")
def ne(mod):
    f = mod[0].NormalEstimation(0)
    yield f
    f.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


class DevArr:
    """a host array uploaded into device memory of an estimator's context (the form of keyframes.DeviceCloud)"""

    def __init__(self, f, a):
        a = np.ascontiguousarray(a, np.float32)
        self._f, self._h, self.n, self.stride_bytes = f, f._h, len(a), a.strides[0]
        self.ptr = f._dev(a.nbytes)
        f._chk(f._L.rgc_upload(f._h, self.ptr, a.ctypes.data, a.nbytes))

    def __len__(self):
        return self.n

    def synchronize(self):
        pass

    def free(self):
        self._f._L.rgc_device_free(self._h, self.ptr)


def estimate(f, cloud, surface, r):
    f.setInputCloud(cloud)
    f.setSearchSurface(surface)
    if r["k"]:
        f.setKSearch(r["k"])
    else:
        f.setRadiusSearch(r["radius"])
    f.setViewPoint(*r["vp"])
    f.setFlip(r["flip"])
    n4 = f.compute(with_moments=True)
    return dict(n4=n4, cov6=f.getCovariances(), cen=f.getCentroids(), cnt=f.getCounts(), n_valid=f.getValidCount(), info=f.info())


def worst(err, tol):
    """the largest err / tol (0 / 0 counts as 0, x / 0 as inf)"""
    err, tol = np.asarray(err, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / tol)
    return float(q.max())


def compare(name, i, got, scale=1.0):
    """the device's result of run i of a case against the reference; scale widens the moments' bounds (2: two radius-route orders against each other's reference)"""
    case, r, ref = CASES[name], CASES[name]["runs"][i], nc.ref(name, i)
    v, n = ref["valid"], len(case["cloud"])
    n4, cov6, cen, cnt = got["n4"], got["cov6"], got["cen"], got["cnt"]
    assert n4.dtype == np.float32 and n4.shape == (n, 4) and cov6.shape == (n, 6) and cen.shape == (n, 3) and cnt.dtype == np.int32
    assert np.array_equal(cnt, ref["count"]), (name, i, np.flatnonzero(cnt != ref["count"])[:10])
    assert got["n_valid"] == ref["n_valid"] == got["info"]["n_valid"]
    assert np.isnan(n4[~v]).all() and np.isnan(cov6[~v]).all() and np.isnan(cen[~v]).all(), "NaN rows exactly where m < 3"
    assert np.isfinite(n4[v]).all() and np.isfinite(cov6[v]).all() and np.isfinite(cen[v]).all()
    figures = {}
    figures["cov"] = worst(np.abs(cov6[v] - ref["cov6"][v]), scale * ref["bound_cov"][v])
    figures["centroid"] = worst(np.abs(cen[v] - ref["centroid"][v]), scale * ref["bound_cen"][v])
    nd = n4[v, :3].astype(np.float64)
    curv = n4[v, 3].astype(np.float64)
    trace_dev = (cov6[v, 0] + cov6[v, 3]) + cov6[v, 5]
    lam = curv * trace_dev
    ev0 = np.abs(ref["ev"][v, 0])
    figures["eigenvalue"] = worst(np.abs(lam - ev0), scale * ref["bound_eig"][v] + 2.0 ** -23 * ev0)
    assert (curv >= 0).all() and (curv[trace_dev <= 0] == 0).all()
    figures["length"] = worst(np.abs(np.sqrt((nd * nd).sum(axis=1)) - 1.0), 2 * 2.0 ** -23)
    S = ref["S"][v]
    resid = np.sqrt(((np.einsum("nij,nj->ni", S, nd) - lam[:, None] * nd) ** 2).sum(axis=1))
    figures["residual"] = worst(resid, 8 * scale * ref["bound_eig"][v] + 2.0 ** -23 * (np.sqrt((S * S).sum(axis=(1, 2))) + lam))
    dec, sure = ref["decided"][v], ref["sign_sure"][v]
    rn, bn = ref["normal"][v], ref["bound_n"][v] * scale
    same = np.abs(nd - rn).max(axis=1)
    either = np.minimum(same, np.abs(nd + rn).max(axis=1))
    figures["normal"] = worst(np.where(sure, same, either)[dec], bn[dec])
    figures["decided"], figures["sign_sure"], figures["valid"] = int(dec.sum()), int(sure.sum()), int(v.sum())
    if "rank" in case["minima"]:
        quad = np.einsum("ni,nij,nj->n", nd, S, nd)
        assert (quad <= 2 * kr.GAP_MIN * ref["trace"][v]).all(), (name, i, quad.max())
    print(name, r, {k: (float("%.3g" % x) if isinstance(x, float) else x) for k, x in figures.items()})
    for what in ("cov", "centroid", "eigenvalue", "length", "residual", "normal"):
        assert figures[what] <= 1.0, (name, i, what, figures[what])
    return figures


@pytest.mark.parametrize("name,i", RUNS)
def test_every_query_equals_the_reference(ne, name, i):
    case, r = CASES[name], CASES[name]["runs"][i]
    route_k = bool(r["k"])
    first = None
    try:
        for cell in (0.0,) + case["cells"]:
            ne.setCell(cell)
            got = estimate(ne, case["cloud"], case["surface"], r)
            info = got["info"]
            assert (info["n"], info["n_surface"], info["route"]) == (len(case["cloud"]), len(nc.surface_of(case)), 0 if route_k else 1)
            assert (info["cell"] == cell or cell == 0.0) and info["cells"] >= 1 and info["candidates"] >= int(got["cnt"].sum()) and (route_k or info["grown"] == 0)
            compare(name, i, got)
            if first is None:
                first = got
            elif route_k:                                     # no output bit of the k route depends on the cell size
                for key in ("n4", "cov6", "cen", "cnt"):
                    assert np.array_equal(bits(got[key]), bits(first[key])), (name, i, cell, key)
            else:                                             # the radius route: the counts do not; the moments' last bits may
                assert np.array_equal(got["cnt"], first["cnt"])
            if name == "sparse":
                assert info["grown"] >= case["minima"]["grown"] > 0
    finally:
        ne.setCell(0.0)
    if case["minima"].get("exact_plane"):
        # the covariance's third row and column are exactly zero: the Jacobi rotations never touch column 2, the solver's normal is +z.  A viewpoint in
        # the plane gives a dot product of exactly 0, which keeps that sign; a viewpoint below the plane flips it; flip = 0 makes z positive
        want = -1.0 if r["flip"] and r["vp"][2] < 0.25 else 1.0
        dec = nc.ref(name, i)["decided"]                      # (rows that are not collinear inside the plane)
        assert dec.sum() >= 0.9 * len(dec) and (first["n4"][dec, :3] == np.array([0.0, 0.0, want], np.float32)).all() and (first["n4"][dec, 3] == 0).all()


@pytest.mark.parametrize("name,i", [("sheet", 0), ("surface", 0), ("tiers", 7)])
def test_the_k_route_gives_identical_bytes_whatever_the_cell_the_pointers_the_strides_and_the_run(ne, name, i):
    case, r = CASES[name], CASES[name]["runs"][i]
    rng = np.random.default_rng(11)
    wide = lambda a: np.concatenate([a, rng.uniform(1, 2, (len(a), 5)).astype(np.float32)], axis=1)
    wq, ws = wide(case["cloud"]), None if case["surface"] is None else wide(case["surface"])
    seen = None
    try:
        for cell in (0.0, 0.0625, 0.25, 1.0):
            ne.setCell(cell)
            for stride_f in (3, 4, 8):
                hq = np.ascontiguousarray(wq[:, :stride_f])
                hs = None if ws is None else np.ascontiguousarray(ws[:, :11 - stride_f])      # (the surface's stride differs from the queries')
                dq, ds = DevArr(ne, hq), None if hs is None else DevArr(ne, hs)
                try:
                    for form, q, s in (("host", hq, hs), ("device", dq, ds), ("host again", hq, hs)):
                        got = estimate(ne, q, s, r)
                        seen = seen or got
                        for key in ("n4", "cov6", "cen", "cnt"):
                            assert np.array_equal(bits(got[key]), bits(seen[key])), (cell, stride_f, form, key)
                        assert got["n_valid"] == seen["n_valid"]
                finally:
                    dq.free()
                    if ds is not None:
                        ds.free()
    finally:
        ne.setCell(0.0)
    compare(name, i, seen)


@pytest.mark.parametrize("name,i", [("sheet", 1), ("surface", 1), ("sweep", 3)])
def test_the_radius_route_is_reproducible_at_a_cell_and_within_the_bound_across_cells(ne, name, i):
    case, r = CASES[name], CASES[name]["runs"][i]
    rng = np.random.default_rng(12)
    wide = lambda a: np.concatenate([a, rng.uniform(1, 2, (len(a), 5)).astype(np.float32)], axis=1)
    wq, ws = wide(case["cloud"]), None if case["surface"] is None else wide(case["surface"])
    per_cell = []
    try:
        for cell in (0.0, 0.125, 0.5, 2.0):
            ne.setCell(cell)
            seen = None
            for stride_f in (3, 4, 8):
                hq = np.ascontiguousarray(wq[:, :stride_f])
                hs = None if ws is None else np.ascontiguousarray(ws[:, :11 - stride_f])
                dq, ds = DevArr(ne, hq), None if hs is None else DevArr(ne, hs)
                try:
                    for form, q, s in (("host", hq, hs), ("device", dq, ds), ("host again", hq, hs)):
                        got = estimate(ne, q, s, r)
                        seen = seen or got
                        for key in ("n4", "cov6", "cen", "cnt"):
                            assert np.array_equal(bits(got[key]), bits(seen[key])), (cell, stride_f, form, key)
                finally:
                    dq.free()
                    if ds is not None:
                        ds.free()
            per_cell.append(seen)
    finally:
        ne.setCell(0.0)
    ref = nc.ref(name, i)
    v = ref["valid"]
    for got in per_cell:
        compare(name, i, got)
        assert np.array_equal(got["cnt"], per_cell[0]["cnt"])
        assert (np.abs(got["cov6"][v] - per_cell[0]["cov6"][v]) <= 2 * ref["bound_cov"][v]).all() and (np.abs(got["cen"][v] - per_cell[0]["cen"][v]) <= 2 * ref["bound_cen"][v]).all()


def test_the_callers_search_index_is_untouched(ne):
    from rgc_slam_amd import search
    tree = search.KdTree(owner=ne)
    tree.setInputCloud(CASES["lattice"]["cloud"])
    q = CASES["tiers"]["cloud"][:150]
    before = tree.nearestKSearch(q, 9) + tree.radiusSearch(q, 0.3)
    info = tree.info()
    estimate(ne, CASES["sheet"]["cloud"], None, CASES["sheet"]["runs"][0])
    estimate(ne, CASES["surface"]["cloud"], CASES["surface"]["surface"], CASES["surface"]["runs"][1])
    after = tree.nearestKSearch(q, 9) + tree.radiusSearch(q, 0.3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    assert (tree.info()["n"], tree.info()["cell"], tree.info()["cells"]) == (info["n"], info["cell"], info["cells"])
    want = sr.knn_rows(CASES["lattice"]["cloud"], q, 9)
    assert np.array_equal(after[0], want[0]) and np.array_equal(bits(after[1]), bits(want[1]))
    tree.clear()


def _params(lib, k=0, radius=0.0, vp=(0.0, 0.0, 0.0), flip=1):
    p = lib.NormalParams()
    lib.load().rgc_default_normal_params(C.byref(p))
    p.k, p.radius, p.flip = k, radius, flip
    p.viewpoint[:] = vp
    return p


def _raw(f, a, n, stride, prm, outs, surface=None, ns=0, sstride=0, n_valid=True, on_device=0):
    p = lambda x: x.ctypes.data if x is not None else None
    return f._L.rgc_normal_estimate(f._h, p(a), n, stride, p(surface), ns, sstride, on_device, C.byref(prm) if prm is not None else None, p(outs["n4"]), p(outs["cov6"]),
                                    p(outs["cen"]), p(outs["cnt"]), C.byref(outs["valid"]) if n_valid else None)


def test_refusals(mod, ne):
    features, lib = mod
    a = np.ascontiguousarray(CASES["tiers"]["cloud"])
    n = len(a)
    outs = dict(n4=np.full((n, 4), 7.5, np.float32), cov6=np.full((n, 6), 7.5), cen=np.full((n, 3), 7.5), cnt=np.full(n, 77, np.int32), valid=C.c_int(-5))
    untouched = lambda: (outs["n4"] == 7.5).all() and (outs["cov6"] == 7.5).all() and (outs["cen"] == 7.5).all() and (outs["cnt"] == 77).all()
    good = _params(lib, k=8)
    assert _raw(ne, a, 0, 12, good, outs) == 0 and outs["valid"].value == 0 and untouched()                    # n = 0
    for bad_value in (np.nan, np.inf, -np.inf):                                                                 # a non-finite coordinate in either cloud: nothing written
        bad = a.copy()
        bad[137, 1] = bad_value
        for prm in (good, _params(lib, radius=0.3)):
            assert _raw(ne, bad, n, 12, prm, outs) == lib.ERR_NONFINITE
            assert _raw(ne, bad, n, 12, prm, outs, surface=a, ns=n, sstride=12) == lib.ERR_NONFINITE             # ... a query
            assert _raw(ne, a, n, 12, prm, outs, surface=bad, ns=n, sstride=12) == lib.ERR_NONFINITE             # ... a surface point
        assert untouched() and outs["valid"].value == 0
    for k, radius in ((0, 0.0), (8, 0.3), (2, 0.0), (33, 0.0), (-1, 0.0), (1, 0.0), (0, -0.3), (0, np.nan), (0, np.inf), (0, 1e30), (0, 1e-30), (8, np.nan)):
        assert _raw(ne, a, n, 12, _params(lib, k=k, radius=radius), outs) == lib.ERR_INVALID, (k, radius)
    for vp in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        assert _raw(ne, a, n, 12, _params(lib, k=8, vp=vp), outs) == lib.ERR_INVALID
    for flip in (2, -1):
        assert _raw(ne, a, n, 12, _params(lib, k=8, flip=flip), outs) == lib.ERR_INVALID
    for stride in (10, 8, 4100):
        assert _raw(ne, a, n, stride, good, outs) == lib.ERR_INVALID
        assert _raw(ne, a, n, 12, good, outs, surface=a, ns=n, sstride=stride) == lib.ERR_INVALID
    assert _raw(ne, None, n, 12, good, outs) == lib.ERR_INVALID and _raw(ne, a, -1, 12, good, outs) == lib.ERR_INVALID    # NULL cloud, n < 0
    assert _raw(ne, a, n, 12, good, outs, surface=a, ns=0, sstride=12) == lib.ERR_INVALID and _raw(ne, a, n, 12, good, outs, surface=a, ns=-3, sstride=12) == lib.ERR_INVALID
    assert _raw(ne, a, n, 12, None, outs) == lib.ERR_INVALID and _raw(ne, a, n, 12, good, outs, n_valid=False) == lib.ERR_INVALID
    assert untouched()
    for cell in (-1.0, np.nan, np.inf):
        assert ne._L.rgc_normal_set_cell(ne._h, cell) == lib.ERR_INVALID
    far = np.concatenate([a, np.array([[9e5, 9e5, 9e4]], np.float32)])                                          # a fixed cell too small for the box; the automatic rule copes
    ne.setCell(0.01)
    try:
        assert _raw(ne, far, n + 1, 12, good, dict(n4=None, cov6=None, cen=None, cnt=None, valid=outs["valid"])) == lib.ERR_GRID_TOO_LARGE
    finally:
        ne.setCell(0.0)
    cnt = np.full(n + 1, 77, np.int32)
    assert _raw(ne, far, n + 1, 12, good, dict(n4=None, cov6=None, cen=None, cnt=cnt, valid=outs["valid"])) == 0 and (cnt == 8).all() and outs["valid"].value == n + 1
    for setter, bads in ((ne.setKSearch, (1, 2, 33, -4)), (ne.setRadiusSearch, (-1.0, float("nan"), float("inf"), 1e30, 1e-30)), (lambda v: ne.setViewPoint(v, 0, 0), (float("nan"), 1e39))):
        for bad in bads:
            with pytest.raises(features.RgcError):
                setter(bad)
    # the next good call after all of that
    compare("tiers", 3, estimate(ne, a, None, CASES["tiers"]["runs"][3]))


def test_a_solve_in_flight_refuses_the_call(mod):
    features, lib = mod
    from rgc_slam_amd import registration, synth
    world, base = synth.make_world_and_map(6000, seed=3)
    base = base.astype(np.float32)
    reg = registration.FastVGICP(0)
    reg.setInputTarget(base)
    reg.setInputSource((base[::3] + np.float32(0.02)).astype(np.float32))
    f = features.NormalEstimation(owner=reg)
    a = np.ascontiguousarray(CASES["tiers"]["cloud"])
    r = CASES["tiers"]["runs"][3]
    before = estimate(f, a, None, r)
    reg.align_begin()
    outs = dict(n4=np.full((len(a), 4), 7.5, np.float32), cov6=None, cen=None, cnt=None, valid=C.c_int(-5))
    assert _raw(f, a, len(a), 12, _params(lib, k=r["k"]), outs) == lib.ERR_INVALID and (outs["n4"] == 7.5).all()
    assert _raw(f, a, len(a), 12, _params(lib, radius=0.3), outs) == lib.ERR_INVALID and (outs["n4"] == 7.5).all()
    reg.align_end()
    after = estimate(f, a, None, r)
    assert np.array_equal(bits(after["n4"]), bits(before["n4"])) and np.array_equal(bits(after["cov6"]), bits(before["cov6"]))
    compare("tiers", 3, after)
    reg.close()


def test_the_python_mirrors_give_the_c_abis_bytes(mod, ne):
    features, lib = mod
    from rgc_slam_amd import odometry
    pre = odometry.Preprocessor(0)
    try:
        for name, i in (("sheet", 2), ("sheet", 4), ("surface", 0), ("surface", 1)):
            case, r = CASES[name], CASES[name]["runs"][i]
            q, s = case["cloud"], case["surface"]
            n = len(q)
            outs = dict(n4=np.empty((n, 4), np.float32), cov6=np.empty((n, 6)), cen=np.empty((n, 3)), cnt=np.empty(n, np.int32), valid=C.c_int(0))
            prm = _params(lib, k=r["k"], radius=r["radius"], vp=r["vp"], flip=int(r["flip"]))
            assert _raw(ne, q, n, 12, prm, outs, surface=s, ns=0 if s is None else len(s), sstride=0 if s is None else 12) == 0
            got = estimate(ne, q, s, r)
            assert np.array_equal(bits(got["n4"]), bits(outs["n4"])) and np.array_equal(bits(got["cov6"]), bits(outs["cov6"])) and np.array_equal(bits(got["cen"]), bits(outs["cen"]))
            assert np.array_equal(got["cnt"], outs["cnt"]) and got["n_valid"] == outs["valid"].value
            only = features.NormalEstimation(owner=ne)
            only.setInputCloud(q)
            only.setSearchSurface(s)
            only.setKSearch(r["k"]) if r["k"] else only.setRadiusSearch(r["radius"])
            only.setViewPoint(*r["vp"])
            only.setFlip(r["flip"])
            assert only.getViewPoint() == tuple(float(np.float32(v)) for v in r["vp"]) and np.array_equal(bits(only.compute()), bits(outs["n4"])) and only.getCovariances() is None
            mine = pre.normalEstimation(q, k=r["k"], radius=r["radius"], viewpoint=r["vp"], surface=s, flip=r["flip"])
            assert mine.dtype == np.float32 and np.array_equal(bits(mine), bits(outs["n4"]))
    finally:
        pre.close()
