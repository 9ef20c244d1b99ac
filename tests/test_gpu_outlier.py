"""The outlier filters (rgc_outlier_*, filters.StatisticalOutlierRemoval / RadiusOutlierRemoval) on the MI355X against the independent numpy reference
tests/outlier_reference.py, on the designed cases of tests/outlier_cases.py (tests/test_outlier_reference.py shows on the CPU what each case contains and
that no point is undecided).

One tolerance appears, and it is derived (outlier_reference.threshold_bound): the device's threshold lies within it of the reference's.  Everything else
is equality: the mean distances bit for bit, the counts, the kept indices -- under the device's OWN threshold and under the reference's mask -- the
records byte for byte, negative as the exact complement; host and device pointers, every stride and every cell size give identical bytes, and so do two
runs.  A reference is computed once per (case, setting) and shared (outlier_cases.ref_sor / ref_counts)."""
import ctypes as C

import numpy as np
import pytest

import outlier_cases as oc
import search_reference as sr

pytestmark = pytest.mark.gpu

CASES = oc.CASES


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, filters
    return filters, _lib


@pytest.fixture(scope="module")
def sor(mod):
    f = mod[0].StatisticalOutlierRemoval(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def ror(mod):
    f = mod[0].RadiusOutlierRemoval(0)
    yield f
    f.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def records(cloud, idx):
    """the 16-byte records the filters emit for input rows idx: x, y, z and the float behind z (0 for a 12-byte stride)"""
    rec = np.zeros((len(idx), 4), np.float32)
    w = min(cloud.shape[1], 4)
    rec[:, :w] = cloud[idx, :w]
    return rec


class DevArr:
    """a host array uploaded into device memory of a filter's context (the form of keyframes.DeviceCloud)"""

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


def run_sor(f, cloud, mean_k, std_mul, negative=False):
    f.setInputCloud(cloud)
    f.setMeanK(mean_k)
    f.setStddevMulThresh(std_mul)
    f.setNegative(negative)
    out = f.filter()
    return out, f.getIndices(), f.getMeanDistances(), f.info()


def run_ror(f, cloud, radius, min_nb, negative=False, with_counts=True):
    f.setInputCloud(cloud)
    f.setRadiusSearch(radius)
    f.setMinNeighborsInRadius(min_nb)
    f.setNegative(negative)
    out = f.filter(with_counts)
    return out, f.getIndices(), f.getCounts(), f.info()


@pytest.mark.parametrize("name", sorted(CASES))
def test_sor_equals_the_reference(sor, name):
    case = CASES[name]
    cloud, n = case["cloud"], len(case["cloud"])
    for mean_k, std_mul in case["sor"]:
        ref = oc.ref_sor(name, mean_k, std_mul)
        out, idx, d, info = run_sor(sor, cloud, mean_k, std_mul)
        bad = np.flatnonzero(bits(d) != bits(ref["d"]))
        assert bad.size == 0, (name, mean_k, bad[:5], d[bad[:5]], ref["d"][bad[:5]])
        gap = abs(np.longdouble(info["threshold"]) - ref["threshold"])
        print(name, "mean_k", mean_k, "threshold", info["threshold"], "|device - reference|", float(gap), "bound", ref["bound"], "cell", info["cell"], "grown", info["grown"],
              "candidates per point %.1f" % (info["candidates"] / n))
        assert gap <= ref["bound"], (name, mean_k, float(gap), ref["bound"])
        assert np.array_equal(idx, np.flatnonzero(d.astype(np.float64) <= info["threshold"])), "the kept set under the device's own threshold"
        assert np.array_equal(idx, np.flatnonzero(ref["inlier"])), "the kept set of the reference"
        assert idx.dtype == np.int32 and out.dtype == np.float32 and np.array_equal(bits(out), bits(records(cloud, idx)))
        assert (info["n"], info["n_out"]) == (n, len(idx)) and info["cells"] >= 1 and info["cell"] > 0 and 0 <= info["grown"] <= n and info["candidates"] >= n * (mean_k + 1)
        assert abs(np.longdouble(info["mean"]) - ref["mean"]) <= ref["bound"]      # (E_mean is one term of the threshold's bound)
        out_n, idx_n, d_n, info_n = run_sor(sor, cloud, mean_k, std_mul, negative=True)
        assert np.array_equal(idx_n, np.setdiff1d(np.arange(n, dtype=np.int32), idx)) and np.array_equal(bits(d_n), bits(d))
        assert np.array_equal(bits(out_n), bits(records(cloud, idx_n))) and bits(np.float64(info_n["threshold"])) == bits(np.float64(info["threshold"]))
        assert np.array_equal(sor.getRemovedIndices(), idx)
    if name == "strays":
        assert info["grown"] >= len(case["strays"]) and not np.isin(case["strays"], idx).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_ror_equals_the_reference(ror, name):
    case = CASES[name]
    cloud, n = case["cloud"], len(case["cloud"])
    for radius, min_nb in case["ror"]:
        want = oc.ref_counts(name, radius)
        keep = np.flatnonzero(want - 1 >= min_nb).astype(np.int32)
        out, idx, cnt, info = run_ror(ror, cloud, radius, min_nb)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, want), (name, radius, np.flatnonzero(cnt != want)[:10])
        assert np.array_equal(idx, keep) and np.array_equal(bits(out), bits(records(cloud, idx)))
        assert (info["n"], info["n_out"], info["threshold"], info["grown"]) == (n, len(keep), 0.0, 0) and info["candidates"] >= int(want.sum())
        exact_candidates = info["candidates"]
        out_e, idx_e, none, info_e = run_ror(ror, cloud, radius, min_nb, with_counts=False)        # the early-exit route keeps the same set
        assert none is None and np.array_equal(idx_e, keep) and np.array_equal(bits(out_e), bits(out)) and n <= info_e["candidates"] <= exact_candidates
        print(name, "r", radius, "min", min_nb, "kept", len(keep), "of", n, "candidates", exact_candidates, "with the early exit", info_e["candidates"])
        for with_counts in (True, False):
            _, idx_n, _, _ = run_ror(ror, cloud, radius, min_nb, negative=True, with_counts=with_counts)
            assert np.array_equal(idx_n, np.setdiff1d(np.arange(n, dtype=np.int32), keep))
    if name == "strays":
        assert (cnt[case["strays"]] == 1).all()


@pytest.mark.parametrize("name", ["lattice", "mid"])
def test_pointers_strides_and_cells_give_identical_bytes(sor, ror, name):
    case = CASES[name]
    n = len(case["cloud"])
    rng = np.random.default_rng(7)
    wide = np.zeros((n, 8), np.float32)
    wide[:, :3] = case["cloud"]
    wide[:, 3:] = rng.uniform(1, 2, (n, 5))                       # c and what lies behind it
    mean_k, std_mul = case["sor"][-1]
    radius, min_nb = case["ror"][-1]
    seen = {}
    try:
        for cell in (0.0, 0.25, 4.0):
            sor.setCell(cell)
            ror.setCell(cell)
            for stride_f in (3, 4, 8):
                host = np.ascontiguousarray(wide[:, :stride_f])
                dev = DevArr(sor, host)
                try:
                    for form, cloud in (("host", host), ("device", dev), ("host again", host)):
                        out, idx, d, info = run_sor(sor, cloud, mean_k, std_mul)
                        assert info["cell"] == cell or cell == 0.0
                        stats = np.array([info["mean"], info["stddev"], info["threshold"]])
                        got = (bits(out[:, :3]), idx, bits(d), bits(stats))
                        assert np.array_equal(bits(out), bits(records(host, idx))), "records go out unchanged, c = 0 for a 12-byte stride"
                        for a, b in zip(got, seen.setdefault("sor", got)):
                            assert np.array_equal(a, b), (cell, stride_f, form)
                finally:
                    dev.free()
                dev = DevArr(ror, host)
                try:
                    for form, cloud in (("host", host), ("device", dev)):
                        out, idx, cnt, info = run_ror(ror, cloud, radius, min_nb)
                        got = (bits(out[:, :3]), idx, cnt)
                        assert np.array_equal(bits(out), bits(records(host, idx)))
                        for a, b in zip(got, seen.setdefault("ror", got)):
                            assert np.array_equal(a, b), (cell, stride_f, form)
                finally:
                    dev.free()
    finally:
        sor.setCell(0.0)
        ror.setCell(0.0)
    ref = oc.ref_sor(name, mean_k, std_mul)
    assert np.array_equal(seen["sor"][2], bits(ref["d"])) and np.array_equal(seen["ror"][2], oc.ref_counts(name, radius))


def test_the_callers_search_index_is_untouched(mod, sor):
    from rgc_slam_amd import search
    case = CASES["mid"]
    tree = search.KdTree(owner=sor)
    tree.setInputCloud(CASES["lattice"]["cloud"])
    q = case["cloud"][:300]
    before = tree.nearestKSearch(q, 9) + tree.radiusSearch(q, 0.3)
    info = tree.info()
    run_sor(sor, case["cloud"], 20, 1.0)
    ror2 = mod[0].RadiusOutlierRemoval(owner=sor)
    run_ror(ror2, case["cloud"], 0.4, 6)
    after = tree.nearestKSearch(q, 9) + tree.radiusSearch(q, 0.3)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    assert (tree.info()["n"], tree.info()["cell"], tree.info()["cells"]) == (info["n"], info["cell"], info["cells"])
    want = sr.knn_rows(CASES["lattice"]["cloud"], q, 9)
    assert np.array_equal(after[0], want[0]) and np.array_equal(bits(after[1]), bits(want[1]))
    tree.clear()


def _raw_sor(f, a, n, stride, mean_k, std_mul, out, idx, d, kept):
    p = lambda x: x.ctypes.data if x is not None else None
    return f._L.rgc_outlier_statistical(f._h, p(a), n, stride, 0, mean_k, std_mul, 0, p(out), p(idx), p(d), C.byref(kept) if kept is not None else None)


def _raw_ror(f, a, n, stride, radius, min_nb, out, idx, cnt, kept):
    p = lambda x: x.ctypes.data if x is not None else None
    return f._L.rgc_outlier_radius(f._h, p(a), n, stride, 0, radius, min_nb, 0, p(out), p(idx), p(cnt), C.byref(kept) if kept is not None else None)


def test_refusals(mod, sor, ror):
    filters, lib = mod
    a = np.ascontiguousarray(CASES["mid"]["cloud"][:200])
    fresh = lambda: (np.full((200, 4), 7.5, np.float32), np.full(200, 77, np.int32), np.full(200, 7.5, np.float32), np.full(200, 77, np.int32))
    out, idx, d, cnt = fresh()
    kept = C.c_int(-5)
    assert _raw_sor(sor, a, 0, 12, 8, 1.0, out, idx, d, kept) == 0 and kept.value == 0              # n = 0
    assert _raw_ror(ror, a, 0, 12, 0.5, 2, out, idx, cnt, kept) == 0 and kept.value == 0
    for bad_value in (np.nan, np.inf, -np.inf):                                                        # a non-finite point: nothing written
        bad = a.copy()
        bad[137, 1] = bad_value
        assert _raw_sor(sor, bad, 200, 12, 8, 1.0, out, idx, d, kept) == lib.ERR_NONFINITE
        assert _raw_ror(ror, bad, 200, 12, 0.5, 2, out, idx, cnt, kept) == lib.ERR_NONFINITE
        assert (out == 7.5).all() and (idx == 77).all() and (d == 7.5).all() and (cnt == 77).all() and kept.value == 0
    for n, mean_k in ((8, 8), (8, 9), (1, 1), (200, 0), (200, -1), (200, 64), (-1, 8)):              # n <= mean_k, n < 2, mean_k out of range
        assert _raw_sor(sor, a, n, 12, mean_k, 1.0, out, idx, d, kept) == lib.ERR_INVALID, (n, mean_k)
    for std_mul in (np.nan, np.inf):
        assert _raw_sor(sor, a, 200, 12, 8, std_mul, out, idx, d, kept) == lib.ERR_INVALID
    for stride in (10, 8, 4100):
        assert _raw_sor(sor, a, 200, stride, 8, 1.0, out, idx, d, kept) == lib.ERR_INVALID
        assert _raw_ror(ror, a, 200, stride, 0.5, 2, out, idx, cnt, kept) == lib.ERR_INVALID
    assert _raw_sor(sor, a, 200, 12, 8, 1.0, out, idx, d, None) == lib.ERR_INVALID                     # NULL n_out, NULL cloud
    assert _raw_sor(sor, None, 200, 12, 8, 1.0, out, idx, d, kept) == lib.ERR_INVALID
    for radius, min_nb in ((0.0, 2), (-1.0, 2), (np.nan, 2), (np.inf, 2), (1e30, 2), (0.5, -1)):
        assert _raw_ror(ror, a, 200, 12, radius, min_nb, out, idx, cnt, kept) == lib.ERR_INVALID, (radius, min_nb)
    assert (out == 7.5).all() and (idx == 77).all() and (d == 7.5).all() and (cnt == 77).all()
    for cell in (-1.0, np.nan, np.inf):
        assert sor._L.rgc_outlier_set_cell(sor._h, cell) == lib.ERR_INVALID
    far = np.concatenate([a, np.array([[9e5, 9e5, 9e4]], np.float32)])                                 # a fixed cell too small for the box; the automatic rule copes
    sor.setCell(0.01)
    try:
        assert _raw_sor(sor, far, 201, 12, 8, 1.0, None, None, None, kept) == lib.ERR_GRID_TOO_LARGE
    finally:
        sor.setCell(0.0)
    idx201 = np.full(201, 77, np.int32)
    assert _raw_sor(sor, far, 201, 12, 8, 1.0, None, idx201, None, kept) == 0 and kept.value >= 190 and 200 not in idx201[:kept.value]
    assert _raw_ror(ror, a, 1, 12, 0.5, 0, out, idx, cnt, kept) == 0 and kept.value == 1 and cnt[0] == 1   # one point: its own only member
    with pytest.raises(filters.RgcError):
        sor.setMeanK(64)
    with pytest.raises(filters.RgcError):
        ror.setRadiusSearch(0.0)
    # the next good call after all of that
    ref_d = __import__("outlier_reference").mean_distances(a, 8)
    _, _, got, _ = run_sor(sor, a, 8, 1.0)
    assert np.array_equal(bits(got), bits(ref_d))


def test_a_solve_in_flight_refuses_the_filters(mod):
    filters, lib = mod
    from rgc_slam_amd import registration, synth
    world, base = synth.make_world_and_map(6000, seed=3)
    base = base.astype(np.float32)
    reg = registration.FastVGICP(0)
    reg.setInputTarget(base)
    reg.setInputSource((base[::3] + np.float32(0.02)).astype(np.float32))
    f, g = filters.StatisticalOutlierRemoval(owner=reg), filters.RadiusOutlierRemoval(owner=reg)
    a = np.ascontiguousarray(CASES["mid"]["cloud"])
    mean_k, std_mul = CASES["mid"]["sor"][0]
    before = run_sor(f, a, mean_k, std_mul)[1]
    reg.align_begin()
    kept = C.c_int(0)
    assert _raw_sor(f, a, len(a), 12, 8, 1.0, None, None, None, kept) == lib.ERR_INVALID
    assert _raw_ror(g, a, len(a), 12, 0.4, 6, None, None, None, kept) == lib.ERR_INVALID
    reg.align_end()
    assert np.array_equal(run_sor(f, a, mean_k, std_mul)[1], before) and np.array_equal(before, np.flatnonzero(oc.ref_sor("mid", mean_k, std_mul)["inlier"]))
    reg.close()
