"""The search index (rgc_search_*, search.KdTree) on the MI355X against the independent numpy reference tests/search_reference.py, on the designed cases
of tests/search_cases.py (tests/test_search_reference.py shows on the CPU what each case contains).

No tolerance appears anywhere: kNN rows, bounded and unbounded sorted radius rows and the offsets EQUAL the reference on every query -- indices as
integers, keys as fp32 bit patterns; an unsorted radius result is compared after a (row, key, index) sort and two runs are identical.  Host and device
pointers, and every cell size, give identical bytes (across cell sizes an unsorted radius result as a set: its order inside a row is the grid's).  The read-outs (grown, rows_sorted_long, candidates) are held to the census: they are the proof of
which route a call took.  A reference row is computed once per (case, k) or (case, r, max_nn) and shared by the tests that need it."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import search_cases as sc
import search_reference as sr

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in sc.all_cases()}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, search
    return search, _lib


@pytest.fixture(scope="module")
def tree(mod):
    t = mod[0].KdTree(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def ref_knn(name, k):
    return sr.knn_rows(CASES[name]["tgt"], CASES[name]["qry"], k)


@functools.lru_cache(maxsize=None)
def ref_radius(name, r, max_nn):
    return sr.radius_csr(CASES[name]["tgt"], CASES[name]["qry"], r, max_nn)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_knn(got, want, what):
    idx, sq = got
    assert idx.dtype == np.int32 and sq.dtype == np.float32 and idx.shape == want[0].shape
    bad = np.flatnonzero((idx != want[0]).any(axis=1) | (bits(sq) != bits(want[1])).any(axis=1))
    assert bad.size == 0, (what, bad[:5], idx[bad[:3]], want[0][bad[:3]], sq[bad[:3]], want[1][bad[:3]])


def same_csr(got, want, what):
    off, idx, sq = got
    assert np.array_equal(off, want[0]), (what, np.flatnonzero(np.diff(off) != np.diff(want[0]))[:10])
    bad = np.flatnonzero((idx != want[1]) | (bits(sq) != bits(want[2])))
    assert bad.size == 0, (what, bad[:10], idx[bad[:10]], want[1][bad[:10]])


class DevArr:
    """a host array uploaded into device memory of a KdTree's context, in the form search.KdTree takes device clouds (keyframes.DeviceCloud's)"""

    def __init__(self, t, a, stride=16):
        a = np.ascontiguousarray(a, np.float32)
        rec = np.zeros((len(a), stride // 4), np.float32)
        rec[:, :3] = a[:, :3]
        self._t, self._h, self.n, self.stride_bytes = t, t._h, len(a), stride
        d = C.c_void_p()
        t._chk(t._L.rgc_device_alloc(t._h, max(rec.nbytes, 16), C.byref(d)))
        if rec.nbytes:
            t._chk(t._L.rgc_upload(t._h, d, rec.ctypes.data, rec.nbytes))
        self.ptr = d

    def __len__(self):
        return self.n

    def synchronize(self):
        pass

    def free(self):
        self._t._L.rgc_device_free(self._h, self.ptr)


@pytest.mark.parametrize("name", sorted(CASES))
def test_knn_rows_equal_the_reference(tree, name):
    case = CASES[name]
    nq, n = len(case["qry"]), len(case["tgt"])
    for cell in (0.0,) + tuple(case["cells"]):
        tree.setInputCloud(case["tgt"], cell)
        info = tree.info()
        assert info["n"] == n and info["cells"] >= 1 and (info["cell"] == cell if cell else info["cell"] > 0)
        for k in case["ks"]:
            same_knn(tree.nearestKSearch(case["qry"], k), ref_knn(name, k), (name, cell, k))
            info = tree.info()
            print(name, "cell", info["cell"], "k", k, "candidates per query %.1f" % (info["candidates"] / nq), "grown", info["grown"])
            assert info["candidates"] >= nq * min(k, n) and 0 <= info["grown"] <= nq and info["rows_sorted_long"] == 0
            if "grow" in case and (k, cell) == case["grow"][:2]:
                must, cannot = sr.grow_census(case["tgt"], case["qry"], k, cell)
                assert must >= case["grow"][2] and must <= info["grown"] <= nq - cannot, (must, cannot, info)


@pytest.mark.parametrize("name", sorted(CASES))
def test_radius_rows_equal_the_reference(mod, tree, name):
    case = CASES[name]
    window = mod[0].sort_window()
    assert case.get("window", window) == window
    for cell in (0.0,) + tuple(case["cells"][:1]):
        tree.setInputCloud(case["tgt"], cell)
        for r, max_nn in case["radii"]:
            want = ref_radius(name, r, max_nn)
            total = int(want[0][-1])
            same_csr(tree.radiusSearch(case["qry"], r, max_nn, True), want, (name, cell, r, max_nn))
            info = tree.info()
            longest = int(np.diff(ref_radius(name, r, 0)[0]).max(initial=0))
            print(name, "cell", info["cell"], "r", r, "max_nn", max_nn, "members", total, "candidates", info["candidates"], "long rows", info["rows_sorted_long"])
            assert info["candidates"] >= total
            assert info["rows_sorted_long"] == (0 if max_nn else int((np.diff(want[0]) > window).sum()))
            if max_nn:
                assert 0 <= info["grown"] <= len(case["qry"])
            a = tree.radiusSearch(case["qry"], r, max_nn, False)
            assert tree.info()["rows_sorted_long"] == 0
            b = tree.radiusSearch(case["qry"], r, max_nn, False)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), "two unsorted runs differ"
            assert np.array_equal(a[0], want[0])
            ga, gw = sr.as_sets(*a), sr.as_sets(*want)
            assert np.array_equal(ga[1], gw[1]) and np.array_equal(bits(ga[2]), bits(gw[2])), (name, r, max_nn, longest)


@pytest.mark.parametrize("nq", sc.NQ_COUNTS)
def test_query_counts(tree, nq):
    case = CASES["lattice"]
    tree.setInputCloud(case["tgt"])
    q = case["qry"][:nq]
    for k in (1, 9, 32):
        want = ref_knn("lattice", k)
        same_knn(tree.nearestKSearch(q, k), (want[0][:nq], want[1][:nq]), (nq, k))
    for max_nn in (0, 5):
        off, idx, key = ref_radius("lattice", 0.125, max_nn)
        same_csr(tree.radiusSearch(q, 0.125, max_nn), (off[:nq + 1], idx[:off[nq]], key[:off[nq]]), (nq, max_nn))


def test_host_and_device_pointers_give_identical_bytes(tree):
    case = CASES["lattice"]
    d_t, d_q = DevArr(tree, case["tgt"], 16), DevArr(tree, case["qry"], 20)
    try:
        for cloud in (case["tgt"], d_t):
            tree.setInputCloud(cloud)
            for q in (case["qry"], d_q):
                same_knn(tree.nearestKSearch(q, 17), ref_knn("lattice", 17), "knn")
                for max_nn, srt in ((0, True), (5, True)):
                    same_csr(tree.radiusSearch(q, 0.125, max_nn, srt), ref_radius("lattice", 0.125, max_nn), ("radius", max_nn))
        h = tree.radiusSearch(case["qry"], 0.125, 0, False)
        d = tree.radiusSearch(d_q, 0.125, 0, False)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(h, d))
    finally:
        d_t.free()
        d_q.free()


def test_every_cell_size_gives_identical_bytes(tree):
    case = CASES["lattice"]
    seen = []
    for cell in (0.0625, 0.25, 1.0, 0.0):
        tree.setInputCloud(case["tgt"], cell)
        u = tree.radiusSearch(case["qry"], 0.125, 0, False)      # (the unsorted order inside a row is the grid's: compared as sets, the offsets as they are)
        seen.append(tree.nearestKSearch(case["qry"], 17) + tree.radiusSearch(case["qry"], 0.125, 0, True) + tree.radiusSearch(case["qry"], 0.125, 5, True)
                    + (u[0],) + tuple(np.ascontiguousarray(x) for x in sr.as_sets(*u)[1:]))
        print("cell", tree.info()["cell"], "cells", tree.info()["cells"])
    for other in seen[1:]:
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(seen[0], other))
    same_knn(seen[0][:2], ref_knn("lattice", 17), "knn")


def _raw_radius(t, q, r, max_nn, srt, off, idx, sq, cap):
    total = C.c_longlong(-1)
    rc = t._L.rgc_search_radius(t._h, q.ctypes.data, len(q), q.strides[0], 0, float(r), max_nn, srt, off.ctypes.data if off is not None else None,
                                idx.ctypes.data if idx is not None else None, sq.ctypes.data if sq is not None else None, cap, C.byref(total))
    return rc, total.value


@pytest.mark.parametrize("max_nn", [0, 5])
def test_the_cap_protocol(mod, tree, max_nn):
    lib = mod[1]
    case = CASES["lattice"]
    tree.setInputCloud(case["tgt"])
    q = np.ascontiguousarray(case["qry"])
    want = ref_radius("lattice", 0.125, max_nn)
    total = int(want[0][-1])
    off, idx, sq = np.full(len(q) + 1, 0x5a5a5a5a, np.int32), np.full(total, 0x5a5a5a5a, np.int32), np.full(total, 7.5, np.float32)
    rc, n = _raw_radius(tree, q, 0.125, max_nn, 1, off, idx, sq, total - 1)
    assert rc == lib.ERR_INVALID and n == total
    assert (off == 0x5a5a5a5a).all() and (idx == 0x5a5a5a5a).all() and (sq == 7.5).all(), "a refused call wrote into the caller's buffers"
    rc, n = _raw_radius(tree, q, 0.125, max_nn, 1, off, idx, sq, total)
    assert rc == 0 and n == total
    same_csr((off, idx, sq), want, "second call")
    rc, n = _raw_radius(tree, q, 0.125, max_nn, 1, off, idx, None, total)       # sq_dist is nullable
    assert rc == 0 and n == total and np.array_equal(idx, want[1])
    rc, n = _raw_radius(tree, q[:0], 0.125, max_nn, 1, off, idx, sq, 0)            # nq = 0
    assert rc == 0 and n == 0 and off[0] == 0


def test_refusals(mod, tree):
    search, lib = mod
    case = CASES["lattice"]
    L, h = tree._L, tree._h
    q = np.ascontiguousarray(case["qry"][:200])
    tree.setInputCloud(case["tgt"])
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = q.copy()
        bad[137, 1] = bad_value
        idx, sq = np.full((200, 5), 77, np.int32), np.full((200, 5), 7.5, np.float32)
        assert L.rgc_search_knn(h, bad.ctypes.data, 200, 12, 0, 5, idx.ctypes.data, sq.ctypes.data) == lib.ERR_NONFINITE
        assert (idx == 77).all() and (sq == 7.5).all()
        for max_nn in (0, 5):
            rc, n = _raw_radius(tree, bad, 0.125, max_nn, 1, None, None, None, 0)
            assert rc == lib.ERR_NONFINITE
        want = ref_knn("lattice", 5)
        same_knn(tree.nearestKSearch(q, 5), (want[0][:200], want[1][:200]), "the next good call")
    # argument errors
    idx, sq = np.zeros((200, 33), np.int32), np.zeros((200, 33), np.float32)
    for k in (0, -1, 33):
        assert L.rgc_search_knn(h, q.ctypes.data, 200, 12, 0, k, idx.ctypes.data, sq.ctypes.data) == lib.ERR_INVALID
    assert L.rgc_search_knn(h, q.ctypes.data, 200, 10, 0, 5, idx.ctypes.data, sq.ctypes.data) == lib.ERR_INVALID
    assert L.rgc_search_knn(h, q.ctypes.data, 200, 12, 0, 5, None, sq.ctypes.data) == lib.ERR_INVALID
    for r, max_nn in ((0.0, 0), (-1.0, 0), (np.nan, 0), (np.inf, 0), (1e30, 0), (0.125, 33), (0.125, -1)):
        assert _raw_radius(tree, q, r, max_nn, 1, None, None, None, 0)[0] == lib.ERR_INVALID, (r, max_nn)
    assert L.rgc_search_knn(h, q.ctypes.data, 0, 12, 0, 5, None, None) == 0     # nq = 0
    # a non-finite indexed point: refused, and the context holds no index
    t = case["tgt"].copy()
    t[11, 2] = np.nan
    assert L.rgc_search_set_cloud(h, t.ctypes.data, len(t), 12, 0, 0.0) == lib.ERR_NONFINITE
    assert tree.info()["n"] == 0
    idx, sq = np.zeros((200, 5), np.int32), np.zeros((200, 5), np.float32)
    assert L.rgc_search_knn(h, q.ctypes.data, 200, 12, 0, 5, idx.ctypes.data, sq.ctypes.data) == lib.ERR_NO_INPUT
    assert L.rgc_search_set_cloud(h, t.ctypes.data, 0, 12, 0, 0.0) == lib.ERR_TOO_FEW_POINTS
    assert L.rgc_search_set_cloud(h, t.ctypes.data, len(t), 12, 0, -1.0) == lib.ERR_INVALID
    far = np.concatenate([case["tgt"], np.array([[9e5, 9e5, 9e4]], np.float32)])
    assert L.rgc_search_set_cloud(h, far.ctypes.data, len(far), 12, 0, 0.01) == lib.ERR_GRID_TOO_LARGE
    tree.setInputCloud(far)                                                      # the automatic rule keeps the grid small
    want = sr.knn_rows(far, q, 5)
    same_knn(tree.nearestKSearch(q, 5), want, "an outlier in the cloud")
    # clear
    tree.setInputCloud(case["tgt"])
    tree.clear()
    assert tree.info()["n"] == 0
    assert L.rgc_search_knn(h, q.ctypes.data, 200, 12, 0, 5, idx.ctypes.data, sq.ctypes.data) == lib.ERR_NO_INPUT
    assert _raw_radius(tree, q, 0.125, 0, 1, None, None, None, 0)[0] == lib.ERR_NO_INPUT


def test_reindexing_and_the_other_subsystems(mod):
    """a smaller and then a larger cloud; on a context that also holds a VGICP source and target an rgc_align before and after a burst of searches returns
    the same bits and the searches are unchanged by the align; queries are refused while a solve is in flight"""
    search, lib = mod
    from rgc_slam_amd import registration, synth
    world, base = synth.make_world_and_map(6000, seed=3)
    base = base.astype(np.float32)
    src = (base[::3] + np.float32(0.02)).astype(np.float32)
    reg = registration.FastVGICP(0)
    reg.setInputTarget(base)
    reg.setInputSource(src)
    reg.align(want_output=False)
    T0 = np.array(reg.getFinalTransformation(), copy=True)
    tree = search.KdTree(owner=reg)
    results = []
    for name in ("lattice", "tiny_5", "lattice", "whole"):
        case = CASES[name]
        tree.setInputCloud(case["tgt"])
        k = case["ks"][-1]
        results.append(tree.nearestKSearch(case["qry"], k))
        same_knn(results[-1], ref_knn(name, k), name)
        r, max_nn = case["radii"][0]
        same_csr(tree.radiusSearch(case["qry"], r, max_nn), ref_radius(name, r, max_nn), name)
    assert np.array_equal(results[0][0], results[2][0])
    reg.align(want_output=False)
    T1 = np.array(reg.getFinalTransformation(), copy=True)
    assert np.array_equal(T0.view(np.uint32), T1.view(np.uint32)), "the searches changed an align"
    case = CASES["whole"]
    same_knn(tree.nearestKSearch(case["qry"], 9), ref_knn("whole", 9), "after the align")
    # between rgc_align_begin and rgc_align_end
    reg.align_begin()
    q = np.ascontiguousarray(case["qry"])
    idx, sq = np.zeros((len(q), 9), np.int32), np.zeros((len(q), 9), np.float32)
    L, h = tree._L, tree._h
    assert L.rgc_search_knn(h, q.ctypes.data, len(q), 12, 0, 9, idx.ctypes.data, sq.ctypes.data) == lib.ERR_INVALID
    assert _raw_radius(tree, q, 1.0, 0, 1, None, None, None, 0)[0] == lib.ERR_INVALID
    assert L.rgc_search_set_cloud(h, q.ctypes.data, len(q), 12, 0, 0.0) == lib.ERR_INVALID
    assert L.rgc_search_clear(h) == lib.ERR_INVALID
    reg.align_end()
    same_knn(tree.nearestKSearch(case["qry"], 9), ref_knn("whole", 9), "after the solve")
    tree.close()
    reg.close()


CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from rgc_slam_amd import _lib, search
t = search.KdTree(0)
a = np.random.default_rng(1).uniform(-1, 1, (500, 3)).astype(np.float32)
L, h = t._L, t._h
assert L.rgc_search_set_cloud(h, a.ctypes.data, 500, 12, 1, 0.0) == _lib.ERR_INVALID, "a host cloud passed as a device cloud"
t.setInputCloud(a)
idx, sq = np.zeros((500, 5), np.int32), np.zeros((500, 5), np.float32)
assert L.rgc_search_knn(h, a.ctypes.data, 500, 12, 1, 5, idx.ctypes.data, sq.ctypes.data) == _lib.ERR_INVALID, "host queries passed as device queries"
total = C.c_longlong(0)
assert L.rgc_search_radius(h, a.ctypes.data, 500, 12, 1, 0.2, 0, 1, None, None, None, 0, C.byref(total)) == _lib.ERR_INVALID
d = C.c_void_p()
assert L.rgc_device_alloc(h, a.nbytes, C.byref(d)) == 0 and L.rgc_upload(h, d, a.ctypes.data, a.nbytes) == 0
assert L.rgc_search_knn(h, d, 500, 12, 1, 5, idx.ctypes.data, sq.ctypes.data) == _lib.ERR_INVALID, "host outputs beside device queries"
assert L.rgc_search_knn(h, d, 501, 12, 1, 5, idx.ctypes.data, sq.ctypes.data) == _lib.ERR_INVALID, "a count beyond the allocation"
i2, s2 = t.nearestKSearch(a, 5)
assert (i2[:, 0] == np.arange(500)).all() and (s2[:, 0] == 0).all()
print("child ok")
"""


def test_check_pointers_in_a_fresh_process():
    """RGC_CHECK_POINTERS=1 is read when a context is created: a fresh child process, in which a host pointer passed as "device" is RGC_ERR_INVALID"""
    env = dict(os.environ, RGC_CHECK_POINTERS="1")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
