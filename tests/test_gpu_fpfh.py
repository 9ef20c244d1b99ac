"""FPFH descriptors (rgc_fpfh_*, features.FPFHEstimation, Preprocessor.fpfhEstimation) on the MI355X against the independent numpy reference
tests/fpfh_reference.py, on the designed cases of tests/fpfh_cases.py (tests/test_fpfh_reference.py shows on the CPU what each case contains).

Equality where the header promises it: the queries' row sizes, the SPFH row sizes with the -1 pattern of a separate surface, n_valid, n_spfh, the NaN rows, and
the SPFH counts of every surface point that owns no undecided pair (a point that owns some: every block still sums to the reference's total, a bin differs by
at most the point's number of undecided pairs).  The descriptors lie within the reference's derived bound (fpfh_reference's docstring) wherever no member owns
an undecided pair; every non-zero block sums to 100 within 11 fp32 ulps of 100.  The bytes are identical across runs, host and device pointers, cloud strides
12 / 16 / 32 and normal strides 12 / 16; the counts (never the floats) across cell sizes.  Each comparison prints its largest error / bound.  A reference is
computed once per case and shared (fpfh_cases.ref)."""
import ctypes as C

import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_reference as fr

pytestmark = pytest.mark.gpu

CASES = fc.cases()
ULP100 = float(np.spacing(np.float32(100.0)))


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, features
    return features, _lib


@pytest.fixture(scope="module")
def fe(mod):
    f = mod[0].FPFHEstimation(0)
    yield f
    f.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


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


def estimate(f, cloud, normals, radius, surface=None):
    f.setInputCloud(cloud)
    f.setSearchSurface(surface)
    f.setInputNormals(normals)
    f.setRadiusSearch(radius)
    out = f.compute(with_spfh=True)
    spfh, scnt = f.getSPFH()
    return dict(fpfh=out, spfh=spfh, spfh_count=scnt, count=f.getCounts(), n_valid=f.getValidCount(), info=f.info())


def run_case(f, name):
    c = CASES[name]
    return estimate(f, c["cloud"], c["normals"], c["radius"], c["surface"])


def compare_ref(label, got, ref, n, ns):
    """the device's result against a reference of fpfh_reference.estimate"""
    out, spfh = got["fpfh"], got["spfh"]
    assert out.dtype == np.float32 and out.shape == (n, 33) and spfh.dtype == np.uint32 and spfh.shape == (ns, 33) and got["count"].dtype == np.int32
    assert np.array_equal(got["count"], ref["count"]), (label, np.flatnonzero(got["count"] != ref["count"])[:10])
    assert np.array_equal(got["spfh_count"], ref["spfh_count"]), (label, np.flatnonzero(got["spfh_count"] != ref["spfh_count"])[:10])
    assert got["n_valid"] == ref["n_valid"] == got["info"]["n_valid"] and got["info"]["n_spfh"] == ref["n_spfh"]
    assert (got["info"]["n"], got["info"]["n_surface"]) == (n, ns)
    comp, und = ref["computed"], ref["spfh_und"]
    assert (spfh[~comp] == 0).all()
    clean = comp & (und == 0)
    assert np.array_equal(spfh[clean].astype(np.int64), ref["spfh"][clean]), (label, np.flatnonzero((spfh.astype(np.int64) != ref["spfh"]).any(axis=1) & clean)[:10])
    owners = np.flatnonzero(comp & (und > 0))
    for s in owners:
        assert np.array_equal(spfh[s].reshape(3, 11).sum(axis=1), ref["spfh"][s].reshape(3, 11).sum(axis=1)) and (np.abs(spfh[s].astype(np.int64) - ref["spfh"][s]) <= und[s]).all(), (label, s)
    if not len(owners):
        assert got["info"]["pairs"] == ref["census"]["computed"] or not comp.all()
    empty = ref["count"] == 0
    assert np.isnan(out[empty]).all() and np.isfinite(out[~empty]).all() and np.array_equal(bits(out[empty]), np.full((int(empty.sum()), 33), 0x7fc00000, np.uint32))
    ok = ~empty & ~ref["tainted"]
    err = np.abs(out[ok].astype(np.float64) - ref["fpfh"][ok])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.where(err == 0, 0.0, err / ref["bound"][ok]).max()) if err.size else 0.0
    sums = out[~empty].astype(np.float64).reshape(-1, 3, 11).sum(axis=2)
    block = float(np.abs(sums[sums != 0] - 100.0).max() / ULP100) if (sums != 0).any() else 0.0
    print(label, dict(queries=n, surface=ns, n_spfh=ref["n_spfh"], pairs=got["info"]["pairs"], owners=len(owners), tainted=int(ref["tainted"].sum()), compared=int(ok.sum()),
                      worst_error_over_bound=float("%.3g" % worst), worst_block_sum_ulps=float("%.3g" % block)))
    assert worst <= 1.0, (label, worst)
    assert block <= 11.0, (label, block)
    assert ((sums != 0) == (ref["fpfh"][~empty].reshape(-1, 3, 11).sum(axis=2) != 0)).all()


def compare(name, got):
    c = CASES[name]
    compare_ref(name, got, fc.ref(name), len(c["cloud"]), len(fc.surface_of(c)))


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_equals_the_reference(fe, name):
    case = CASES[name]
    first = None
    try:
        for cell in (0.0,) + case["cells"]:
            fe.setCell(cell)
            got = run_case(fe, name)
            info = got["info"]
            assert (info["cell"] == cell or cell == 0.0) and info["cells"] >= 1 and info["candidates"] >= int(got["count"].sum())
            compare(name, got)
            if first is None:
                first = got
            else:                                             # the counts do not depend on the cell size; the descriptors' last bits may
                for key in ("spfh", "spfh_count", "count"):
                    assert np.array_equal(got[key], first[key]), (name, cell, key)
    finally:
        fe.setCell(0.0)
    if name == "one_cell":
        fe.setCell(64.0)
        try:
            assert run_case(fe, name)["info"]["cells"] <= 8
        finally:
            fe.setCell(0.0)


@pytest.mark.parametrize("name", ["sphere", "keypoints", "plane_nan"])
def test_identical_bytes_whatever_the_run_the_pointers_and_the_strides_and_identical_counts_whatever_the_cell(fe, name):
    case = CASES[name]
    rng = np.random.default_rng(13)
    wide = lambda a: np.concatenate([a, rng.uniform(1, 2, (len(a), 5)).astype(np.float32)], axis=1)
    wq, ws, wn = wide(case["cloud"]), None if case["surface"] is None else wide(case["surface"]), wide(case["normals"])
    per_cell = []
    try:
        for cell in (0.0, 0.0625, 0.25, 1.0):
            fe.setCell(cell)
            seen = None
            for stride_f, nstride_f in ((3, 3), (4, 4), (8, 3), (3, 4)):
                hq = np.ascontiguousarray(wq[:, :stride_f])
                hs = None if ws is None else np.ascontiguousarray(ws[:, :11 - stride_f])      # (the surface's stride differs from the queries')
                hn = np.ascontiguousarray(wn[:, :nstride_f])
                dq, ds, dn = DevArr(fe, hq), None if hs is None else DevArr(fe, hs), DevArr(fe, hn)
                try:
                    for form, q, s, nr in (("host", hq, hs, hn), ("device", dq, ds, dn), ("host again", hq, hs, hn)):
                        got = estimate(fe, q, nr, case["radius"], s)
                        seen = seen or got
                        for key in ("fpfh", "spfh", "spfh_count", "count"):
                            assert np.array_equal(bits(got[key]), bits(seen[key])), (cell, stride_f, nstride_f, form, key)
                        assert got["n_valid"] == seen["n_valid"]
                finally:
                    dq.free()
                    dn.free()
                    if ds is not None:
                        ds.free()
            per_cell.append(seen)
    finally:
        fe.setCell(0.0)
    for got in per_cell:
        compare(name, got)
        for key in ("spfh", "spfh_count", "count"):
            assert np.array_equal(got[key], per_cell[0][key])


def test_normals_computed_on_the_device_are_consumed_without_a_host_trip(mod, fe):
    features, lib = mod
    cloud = CASES["sphere"]["cloud"]
    n = len(cloud)
    ne = features.NormalEstimation(owner=fe)
    dc = DevArr(fe, cloud)
    d_n4 = fe._dev(16 * n)
    try:
        prm = lib.NormalParams()
        lib.load().rgc_default_normal_params(C.byref(prm))
        prm.radius = 0.15
        prm.viewpoint[:] = (0.0, 0.0, 0.0)
        valid = C.c_int(0)
        ne._chk(ne._L.rgc_normal_estimate(ne._h, dc.ptr, n, 12, None, 0, 0, 1, C.byref(prm), d_n4, None, None, None, C.byref(valid)))
        n4 = np.empty((n, 4), np.float32)
        fe._down(n4, d_n4)                                   # (for the reference only)
        assert 0 < valid.value <= n

        class Normals:                                       # out_normal4 where rgc_normal_estimate left it: 16-byte rows on the device
            ptr, stride_bytes, _h = d_n4, 16, fe._h

            def __len__(self):
                return n

            def synchronize(self):
                pass

        got = estimate(fe, dc, Normals(), 0.2)
        ref = fr.estimate(cloud, n4, 0.2)
        assert ref["census"]["owners"] <= 0.001 * n and ref["census"]["pairs"] > 80000
        compare_ref("device normals", got, ref, n, n)
        host = estimate(fe, cloud, n4, 0.2)
        for key in ("fpfh", "spfh", "spfh_count", "count"):
            assert np.array_equal(bits(got[key]), bits(host[key])), key
    finally:
        dc.free()
        fe._L.rgc_device_free(fe._h, d_n4)


def _params(lib, radius):
    p = lib.FpfhParams()
    lib.load().rgc_default_fpfh_params(C.byref(p))
    p.radius = radius
    return p


def _raw(f, a, n, stride, normals, nstride, prm, outs, surface=None, ns=0, sstride=0, n_valid=True):
    p = lambda x: x.ctypes.data if x is not None else None
    return f._L.rgc_fpfh_estimate(f._h, p(a), n, stride, p(surface), ns, sstride, p(normals), nstride, 0, C.byref(prm) if prm is not None else None, p(outs["fpfh"]),
                                  p(outs["spfh"]), p(outs["scnt"]), p(outs["cnt"]), C.byref(outs["valid"]) if n_valid else None)


def test_refusals_and_the_next_valid_call_after_each(mod, fe):
    features, lib = mod
    case = CASES["one_cell"]
    a, nr, r = case["cloud"], case["normals"], case["radius"]
    n = len(a)
    outs = dict(fpfh=np.full((n, 33), 7.5, np.float32), spfh=np.full((n, 33), 77, np.uint32), scnt=np.full(n, 77, np.int32), cnt=np.full(n, 77, np.int32), valid=C.c_int(-5))
    untouched = lambda: (outs["fpfh"] == 7.5).all() and (outs["spfh"] == 77).all() and (outs["scnt"] == 77).all() and (outs["cnt"] == 77).all()
    good = _params(lib, r)
    ref = fc.ref("one_cell")

    def then_a_valid_call_is_correct():
        res = dict(fpfh=np.empty((n, 33), np.float32), spfh=np.empty((n, 33), np.uint32), scnt=np.empty(n, np.int32), cnt=np.empty(n, np.int32), valid=C.c_int(-1))
        assert _raw(fe, a, n, 12, nr, 12, good, res) == 0
        assert np.array_equal(res["cnt"], ref["count"]) and np.array_equal(res["scnt"], ref["spfh_count"]) and np.array_equal(res["spfh"].astype(np.int64), ref["spfh"])
        assert res["valid"].value == ref["n_valid"] and (np.abs(res["fpfh"].astype(np.float64) - ref["fpfh"]) <= ref["bound"]).all()

    assert ref["census"]["owners"] == 0
    assert _raw(fe, a, 0, 12, nr, 12, good, outs) == 0 and outs["valid"].value == 0 and untouched()                 # n = 0
    refused = []
    for radius in (0.0, -0.05, np.nan, np.inf, -np.inf, 1e30, 1e-30):
        refused.append(lambda radius=radius: _raw(fe, a, n, 12, nr, 12, _params(lib, radius), outs))
    for stride in (10, 8, 4100):
        refused.append(lambda stride=stride: _raw(fe, a, n, stride, nr, 12, good, outs))
        refused.append(lambda stride=stride: _raw(fe, a, n, 12, nr, stride, good, outs))
        refused.append(lambda stride=stride: _raw(fe, a, n, 12, nr, 12, good, outs, surface=a, ns=n, sstride=stride))
    refused.append(lambda: _raw(fe, None, n, 12, nr, 12, good, outs))                                                # NULL cloud
    refused.append(lambda: _raw(fe, a, n, 12, None, 12, good, outs))                                                 # NULL normals
    refused.append(lambda: _raw(fe, a, -1, 12, nr, 12, good, outs))                                                  # n < 0
    refused.append(lambda: _raw(fe, a, n, 12, nr, 12, good, outs, surface=a, ns=0, sstride=12))
    refused.append(lambda: _raw(fe, a, n, 12, nr, 12, good, outs, surface=a, ns=-3, sstride=12))
    refused.append(lambda: _raw(fe, a, n, 12, nr, 12, None, outs))                                                   # NULL params
    refused.append(lambda: _raw(fe, a, n, 12, nr, 12, good, outs, n_valid=False))                                    # NULL n_valid
    refused.append(lambda: _raw(fe, a, (1 << 27) + 1, 12, nr, 12, good, outs))                                       # beyond 2^27 points (refused before anything is read)
    refused.append(lambda: _raw(fe, a, n, 12, nr, 12, good, outs, surface=a, ns=(1 << 27) + 1, sstride=12))
    for call in refused:
        assert call() == lib.ERR_INVALID
        assert untouched() and outs["valid"].value in (-5, 0)
        then_a_valid_call_is_correct()
    for cell in (-1.0, np.nan, np.inf):
        assert fe._L.rgc_fpfh_set_cell(fe._h, cell) == lib.ERR_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30, 1e-30):
        with pytest.raises(features.RgcError):
            fe.setRadiusSearch(bad)
    then_a_valid_call_is_correct()


def test_a_non_finite_coordinate_is_refused_and_a_non_finite_normal_is_data(mod, fe):
    features, lib = mod
    case = CASES["one_cell"]
    a, nr, r = case["cloud"], case["normals"], case["radius"]
    n = len(a)
    outs = dict(fpfh=np.full((n, 33), 7.5, np.float32), spfh=None, scnt=None, cnt=np.full(n, 77, np.int32), valid=C.c_int(-5))
    good = _params(lib, r)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = a.copy()
        bad[137, 1] = bad_value
        assert _raw(fe, bad, n, 12, nr, 12, good, outs) == lib.ERR_NONFINITE                                         # the cloud, its own surface
        assert _raw(fe, bad, n, 12, nr, 12, good, outs, surface=a, ns=n, sstride=12) == lib.ERR_NONFINITE            # ... a query
        assert _raw(fe, a, n, 12, nr, 12, good, outs, surface=bad, ns=n, sstride=12) == lib.ERR_NONFINITE            # ... a surface point
        assert (outs["fpfh"] == 7.5).all() and (outs["cnt"] == 77).all() and outs["valid"].value == 0
    compare("one_cell", run_case(fe, "one_cell"))
    nb = nr.copy()
    nb[137] = np.nan
    got = estimate(fe, a, nb, r)
    compare_ref("a NaN normal", got, fr.estimate(a, nb, r), n, n)
    assert (got["spfh"][137] == 0).all() and got["spfh_count"][137] >= 1


def test_a_solve_in_flight_refuses_the_call(mod):
    features, lib = mod
    from rgc_slam_amd import registration, synth
    world, base = synth.make_world_and_map(6000, seed=3)
    base = base.astype(np.float32)
    reg = registration.FastVGICP(0)
    reg.setInputTarget(base)
    reg.setInputSource((base[::3] + np.float32(0.02)).astype(np.float32))
    f = features.FPFHEstimation(owner=reg)
    case = CASES["one_cell"]
    a, nr, r = case["cloud"], case["normals"], case["radius"]
    before = estimate(f, a, nr, r)
    reg.align_begin()
    outs = dict(fpfh=np.full((len(a), 33), 7.5, np.float32), spfh=None, scnt=None, cnt=None, valid=C.c_int(-5))
    assert _raw(f, a, len(a), 12, nr, 12, _params(lib, r), outs) == lib.ERR_INVALID and (outs["fpfh"] == 7.5).all()
    reg.align_end()
    after = estimate(f, a, nr, r)
    assert np.array_equal(bits(after["fpfh"]), bits(before["fpfh"])) and np.array_equal(after["spfh"], before["spfh"])
    compare("one_cell", after)
    reg.close()


def test_the_python_mirrors_give_the_c_abis_bytes(mod, fe):
    features, lib = mod
    from rgc_slam_amd import odometry
    pre = odometry.Preprocessor(0)
    try:
        for name in ("plane", "keypoints"):
            case = CASES[name]
            q, s, nr = case["cloud"], case["surface"], case["normals"]
            n, ns = len(q), len(fc.surface_of(case))
            outs = dict(fpfh=np.empty((n, 33), np.float32), spfh=np.empty((ns, 33), np.uint32), scnt=np.empty(ns, np.int32), cnt=np.empty(n, np.int32), valid=C.c_int(0))
            assert _raw(fe, q, n, 12, nr, 12, _params(lib, case["radius"]), outs, surface=s, ns=0 if s is None else ns, sstride=0 if s is None else 12) == 0
            got = run_case(fe, name)
            assert np.array_equal(bits(got["fpfh"]), bits(outs["fpfh"])) and np.array_equal(got["spfh"], outs["spfh"]) and np.array_equal(got["spfh_count"], outs["scnt"])
            assert np.array_equal(got["count"], outs["cnt"]) and got["n_valid"] == outs["valid"].value
            only = features.FPFHEstimation(owner=fe)
            only.setInputCloud(q)
            only.setSearchSurface(s)
            only.setInputNormals(nr)
            only.setRadiusSearch(case["radius"])
            assert np.array_equal(bits(only.compute()), bits(outs["fpfh"])) and only.getSPFH() == (None, None) and np.array_equal(only.getCounts(), outs["cnt"])
            mine = pre.fpfhEstimation(q, nr, case["radius"], surface=s)
            assert mine.dtype == np.float32 and np.array_equal(bits(mine), bits(outs["fpfh"]))
    finally:
        pre.close()
