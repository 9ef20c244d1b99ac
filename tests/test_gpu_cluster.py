"""Euclidean cluster extraction (rgc_cluster_*, segmentation.EuclideanClusterExtraction) on the MI355X against the independent numpy / scipy reference
tests/cluster_reference.py, on the designed cases of tests/cluster_cases.py (tests/test_cluster_reference.py shows on the CPU what each case contains and
that the reference's components are PCL's clusters).

No tolerance appears: every output is compared for EQUALITY -- the labels, the offsets, the indices, the number of clusters, the info counts -- and the
entries behind the ranges the call owns must keep what the caller put there.  Every designed case runs at four cell sizes of the call's grid (tolerance /
8, tolerance, 8 x tolerance, automatic); host and device pointers, every stride, every subset of outputs and two runs give identical bytes.  A reference
is computed once per (case, tolerance, limits) and shared (cluster_cases.ref)."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as cc
import cluster_reference as cr

pytestmark = pytest.mark.gpu

INT_MAX = cc.INT_MAX
SENTINEL = -77


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, segmentation
    return segmentation, _lib


@pytest.fixture(scope="module")
def ec(mod):
    f = mod[0].EuclideanClusterExtraction(0)
    yield f
    f.close()


def raw(f, a, tol, lo=1, hi=INT_MAX, want=(True, True, True), n=None, stride=None, m=True):
    """rgc_cluster_extract on host memory: (rc, n_clusters, labels, offsets, indices), the arrays pre-filled with SENTINEL (None where not asked for)"""
    n = len(a) if n is None else n
    size = max(len(a) if a is not None else 0, n, 0)
    out = [np.full(size + extra, SENTINEL, np.int32) if w else None for w, extra in zip(want, (0, 1, 0))]
    p = lambda x: x.ctypes.data if x is not None else None
    k = C.c_int(-5)
    rc = f._L.rgc_cluster_extract(f._h, p(a), n, a.strides[0] if stride is None else stride, 0, float(tol), lo, hi, p(out[0]), p(out[1]), p(out[2]), C.byref(k) if m else None)
    return (rc, k.value) + tuple(out)


def check(got, ref, what):
    rc, m, labels, offsets, indices = got
    assert rc == 0 and m == ref["n_clusters"], (what, rc, m, ref["n_clusters"])
    nc = ref["n_clustered"]
    if labels is not None:
        assert np.array_equal(labels, ref["labels"]), (what, np.flatnonzero(labels != ref["labels"])[:8])
    if offsets is not None:
        assert np.array_equal(offsets[:m + 1], ref["offsets"]) and (offsets[m + 1:] == SENTINEL).all(), what
    if indices is not None:
        assert np.array_equal(indices[:nc], ref["indices"]) and (indices[nc:] == SENTINEL).all(), what


def check_info(f, ref, what, cell=0.0):
    info = f.info()
    for k in ("n", "n_components", "n_clusters", "n_clustered", "largest"):
        assert info[k] == ref[k], (what, k, info[k], ref[k])
    assert info["candidates"] >= ref["edges"] and info["cells"] >= 1 and (info["cell"] == cell or (cell == 0.0 and info["cell"] > 0)), (what, info)
    return info


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_every_designed_case_equals_the_reference_at_every_cell_size(ec, name):
    case = cc.CASES[name]
    a = case["cloud"]
    try:
        for tol in case["tol"]:
            for lo, hi in case["limits"]:
                ref = cc.ref(name, tol, lo, hi)
                for cell in (tol / 8, tol, 8 * tol, 0.0):
                    ec.setCell(cell)
                    check(raw(ec, a, tol, lo, hi), ref, (name, tol, lo, hi, cell))
                    info = check_info(ec, ref, (name, tol, lo, hi, cell), cell)
                print(name, "tol", tol, "limits", (lo, hi), "clusters", ref["n_clusters"], "of", ref["n_components"], "components, largest", ref["largest"], "edges", ref["edges"],
                      "automatic cell", info["cell"], "candidates per point %.1f" % (info["candidates"] / max(len(a), 1)))
    finally:
        ec.setCell(0.0)
    for k, v in case["minima"].items():           # (the case contains what it was designed to: the reference's count, as tests/test_cluster_reference.py)
        assert cc.ref(name, case["tol"][0], *case["limits"][0])[k] >= v


@pytest.mark.parametrize("name", ["blobs_2000", "blobs_30000", "scan"])
def test_general_position(ec, name):
    case = cc.case(name)
    a = case["cloud"]
    for tol in case["tol"]:
        for lo, hi in case["limits"]:
            ref = cc.ref(name, tol, lo, hi)
            check(raw(ec, a, tol, lo, hi), ref, (name, tol, lo, hi))
            check_info(ec, ref, (name, tol, lo, hi))
            print(name, "tol", tol, "limits", (lo, hi), "clusters", ref["n_clusters"], "of", ref["n_components"], "components, largest", ref["largest"], "ties", ref["ties"])
    mid = cc.ref(name, case["tol"][1], *case["limits"][1])       # (the case is no trivial one: many clusters, and the limits drop components)
    assert cc.ref(name, case["tol"][1])["n_clusters"] > 10 and mid["over"] + mid["under"] > 0 and mid["n_clusters"] > 1


class DevBuf:
    """host data in device memory of the extractor's context"""

    def __init__(self, f, a):
        a = np.ascontiguousarray(a)
        self._f, self.host = f, a
        self.ptr = f._dev(a.nbytes)
        f._chk(f._L.rgc_upload(f._h, self.ptr, a.ctypes.data, a.nbytes))

    def down(self):
        out = np.empty_like(self.host)
        self._f._down(out, self.ptr)
        return out

    def free(self):
        self._f._L.rgc_device_free(self._f._h, self.ptr)


def raw_device(f, a, tol, lo, hi, want=(True, True, True)):
    n = len(a)
    bufs = [DevBuf(f, a)] + [DevBuf(f, np.full(n + extra, SENTINEL, np.int32)) if w else None for w, extra in zip(want, (0, 1, 0))]
    try:
        k = C.c_int(-5)
        rc = f._L.rgc_cluster_extract(f._h, bufs[0].ptr, n, a.strides[0], 1, float(tol), lo, hi, *[b.ptr if b else None for b in bufs[1:]], C.byref(k))
        return (rc, k.value) + tuple(b.down() if b else None for b in bufs[1:])
    finally:
        for b in bufs:
            if b:
                b.free()


@pytest.mark.parametrize("name,tol,lo,hi", [("limits", 0.5, 2, 7), ("helix_257_shuf", 0.5, 1, INT_MAX), ("lattice_iso", 0.5, 1, INT_MAX), ("double_helix", 0.5, 1, INT_MAX)])
def test_pointers_strides_and_absent_outputs_give_identical_bytes(ec, name, tol, lo, hi):
    case = cc.CASES[name]
    n = len(case["cloud"])
    ref = cc.ref(name, tol, lo, hi)
    rng = np.random.default_rng(11)
    wide = np.zeros((n, 8), np.float32)
    wide[:, :3] = case["cloud"]
    wide[:, 3:] = rng.uniform(1, 2, (n, 5))                       # what lies behind z is not read
    for stride_f in (3, 4, 8):
        host = np.ascontiguousarray(wide[:, :stride_f])
        check(raw(ec, host, tol, lo, hi), ref, (name, "host", stride_f))
        check(raw_device(ec, host, tol, lo, hi), ref, (name, "device", stride_f))
    host = np.ascontiguousarray(wide[:, :4])
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (False, True, False), (True, False, False), (False, False, False)):
        check(raw(ec, host, tol, lo, hi, want), ref, (name, "host", want))
        check_info(ec, ref, (name, want))
        check(raw_device(ec, host, tol, lo, hi, want), ref, (name, "device", want))


def test_twice_on_one_context_and_after_a_larger_cloud(ec):
    order = [("limits", 0.5, 2, 7), ("helix_4097_shuf", 0.5, 1, INT_MAX), ("limits", 0.5, 2, 7), ("lattice_iso", 0.5, 1, INT_MAX), ("limits", 0.5, 8, 8), ("thr_origin", 0.5, 1, INT_MAX),
             ("limits", 0.5, 2, 7), ("chain_1", 0.5, 1, INT_MAX)]
    for name, tol, lo, hi in order + order:
        check(raw(ec, cc.CASES[name]["cloud"], tol, lo, hi), cc.ref(name, tol, lo, hi), (name, lo, hi))
        check_info(ec, cc.ref(name, tol, lo, hi), name)


def test_refusals(mod, ec):
    seg, lib = mod
    a = np.ascontiguousarray(cc.CASES["limits"]["cloud"])
    n = len(a)
    untouched = lambda got: all((x == SENTINEL).all() for x in got[2:] if x is not None)
    got = raw(ec, a, 0.5, n=0)                                                                           # n = 0: zero clusters, offsets[0] = 0
    assert got[:2] == (0, 0) and got[3][0] == 0 and (got[3][1:] == SENTINEL).all() and (got[2] == SENTINEL).all() and (got[4] == SENTINEL).all()
    assert raw(ec, a, 0.5, n=0, want=(False, False, False))[:2] == (0, 0)
    assert ec.info()["n"] == 0 and ec.info()["n_clusters"] == 0
    for bad_value in (np.nan, np.inf, -np.inf):                                                           # a non-finite point: nothing written
        bad = a.copy()
        bad[137, 1] = bad_value
        got = raw(ec, bad, 0.5)
        assert got[0] == lib.ERR_NONFINITE and got[1] == 0 and untouched(got)
        check(raw(ec, a, 0.5, 2, 7), cc.ref("limits", 0.5, 2, 7), "the next call after a refusal")
    for tol in (0.0, -1.0, np.nan, np.inf, 1e30):
        got = raw(ec, a, tol)
        assert got[0] == lib.ERR_INVALID and untouched(got), tol
    for lo, hi in ((0, 5), (-1, 5), (5, 4), (1, 0)):
        got = raw(ec, a, 0.5, lo, hi)
        assert got[0] == lib.ERR_INVALID and untouched(got), (lo, hi)
    for stride in (10, 8, 4100):
        got = raw(ec, a, 0.5, stride=stride)
        assert got[0] == lib.ERR_INVALID and untouched(got), stride
    got = raw(ec, a, 0.5, n=-1)
    assert got[0] == lib.ERR_INVALID and untouched(got)
    got = raw(ec, a, 0.5, m=False)                                                                        # NULL n_clusters
    assert got[0] == lib.ERR_INVALID and untouched(got)
    k = C.c_int(-5)
    assert ec._L.rgc_cluster_extract(ec._h, None, n, 12, 0, 0.5, 1, INT_MAX, None, None, None, C.byref(k)) == lib.ERR_INVALID and k.value == -5    # NULL cloud
    for cell in (-1.0, np.nan, np.inf):
        assert ec._L.rgc_cluster_set_cell(ec._h, cell) == lib.ERR_INVALID
    far = np.concatenate([a, np.array([[9e5, 9e5, 9e4]], np.float32)])                                    # a fixed cell too small for the box; the automatic rule copes
    ec.setCell(0.01)
    try:
        got = raw(ec, far, 0.5)
        assert got[0] == lib.ERR_GRID_TOO_LARGE and untouched(got)
    finally:
        ec.setCell(0.0)
    check(raw(ec, far, 0.5), cr.extract(far, 0.5), "the automatic cell copes with a far point")
    check(raw(ec, a, 0.5, 1, INT_MAX), cc.ref("limits", 0.5), "PCL's defaults are accepted")
    for bad in (0.0, -1.0, float("nan"), 1e30):
        with pytest.raises(seg.RgcError):
            ec.setClusterTolerance(bad)
    with pytest.raises(seg.RgcError):
        ec.setMinClusterSize(0)


def test_a_solve_in_flight_refuses_and_the_neighbours_are_untouched(mod):
    seg, lib = mod
    from rgc_slam_amd import registration, search, synth
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64 if x.dtype.itemsize == 8 else np.uint32)
    world, base = synth.make_world_and_map(6000, seed=3)
    base = base.astype(np.float32)
    reg = registration.FastVGICP(0)
    reg.setInputTarget(base)
    reg.setInputSource((base[::3] + np.float32(0.02)).astype(np.float32))
    tree = search.KdTree(owner=reg)
    tree.setInputCloud(cc.CASES["lattice_iso"]["cloud"])
    q = cc.CASES["limits"]["cloud"][:100] + np.float32(0.1)
    before = list(tree.nearestKSearch(q, 9)) + list(tree.radiusSearch(q, 0.8)) + [reg.getSourceCovariances(), reg.getTargetCovariances(), np.array([reg.fitnessAt(np.eye(4))])]
    tree_info = tree.info()
    f = seg.EuclideanClusterExtraction(owner=reg)
    a = cc.CASES["limits"]["cloud"]
    check(raw(f, a, 0.5, 2, 7), cc.ref("limits", 0.5, 2, 7), "in a registration's context")
    check(raw(f, cc.CASES["helix_4097_shuf"]["cloud"], 0.5), cc.ref("helix_4097_shuf", 0.5), "a larger cloud in a registration's context")
    after = list(tree.nearestKSearch(q, 9)) + list(tree.radiusSearch(q, 0.8)) + [reg.getSourceCovariances(), reg.getTargetCovariances(), np.array([reg.fitnessAt(np.eye(4))])]
    assert len(before) == len(after) and all(np.array_equal(bits(np.asarray(x)), bits(np.asarray(y))) for x, y in zip(before, after))
    assert {k: tree.info()[k] for k in ("n", "cell", "cells")} == {k: tree_info[k] for k in ("n", "cell", "cells")}
    reg.align_begin()
    got = raw(f, a, 0.5, 2, 7)
    assert got[0] == lib.ERR_INVALID and all((x == SENTINEL).all() for x in got[2:])
    reg.align_end()
    check(raw(f, a, 0.5, 2, 7), cc.ref("limits", 0.5, 2, 7), "after the solve")
    tree.clear()
    reg.close()


def test_the_mirrors_return_the_c_abis_rows(mod, ec):
    seg, lib = mod
    from rgc_slam_amd import odometry
    name, tol, lo, hi = "limits", 0.5, 2, 7
    a = cc.CASES[name]["cloud"]
    ref = cc.ref(name, tol, lo, hi)
    rc, m, labels, offsets, indices = raw(ec, a, tol, lo, hi)
    ec.setInputCloud(a)
    ec.setClusterTolerance(tol)
    ec.setMinClusterSize(lo)
    ec.setMaxClusterSize(hi)
    assert (ec.getClusterTolerance(), ec.getMinClusterSize(), ec.getMaxClusterSize()) == (tol, lo, hi)
    for form in ("host", "device"):
        dev = DevBuf(ec, a) if form == "device" else None
        try:
            if dev:
                class Cloud:
                    ptr, stride_bytes, _h = dev.ptr, 12, ec._h
                    __len__ = lambda self: len(a)
                    synchronize = lambda self: None
                ec.setInputCloud(Cloud())
            rows = ec.extract()
            assert len(rows) == m == ref["n_clusters"] and all(r.dtype == np.int32 and np.array_equal(r, w) for r, w in zip(rows, cr.rows(ref)))
            assert np.array_equal(ec.labels(), labels) and np.array_equal(ec.offsets(), offsets[:m + 1]) and np.array_equal(ec.indices(), indices[:ref["n_clustered"]])
            assert ec.info()["n_clusters"] == m
        finally:
            if dev:
                dev.free()
    pre = odometry.Preprocessor(0)
    try:
        got = pre.euclideanClusterExtraction(a, tol, lo, hi)
        assert all(np.array_equal(x, y) and x.dtype == np.int32 for x, y in zip(got, (ref["labels"], ref["offsets"], ref["indices"])))
        d = pre.euclideanClusterExtraction(a, tol)
        assert np.array_equal(d[0], cc.ref(name, tol)["labels"])
    finally:
        pre.close()
