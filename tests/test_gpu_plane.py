"""RANSAC plane segmentation (rgc_plane_*, segmentation.SACSegmentation) on the MI355X against the independent numpy reference tests/plane_reference.py, on
the designed cases of tests/plane_cases.py (tests/test_plane_reference.py shows on the CPU what each case contains and that it is decidable).

Everything is compared for EQUALITY except the refined coefficients: out_counts position by position, iterations, skipped, positions, best_position,
best_count, the RANSAC coefficients before refinement, the inlier indices, the records; the entries behind the written ranges must keep a sentinel.  The
refined coefficients are held to the DERIVED bound of plane_reference.refine (the fixed-order sums' backward error through the eigen gap, times 8) plus the
float32 rounding of the result -- the measured error is printed beside it -- and the re-selected inlier set is compared for equality where the reference
shows no point nearer to the threshold than that bound allows (plane_cases.tolerances); every case runs with optimize = 0 as well, where the set is always
compared.  On every case and every variant the score rule applied in numpy float32 to the REPORTED coefficients reproduces the reported set exactly.

Every case runs at batch sizes 1, 7, 64 and automatic with host and with device pointers, twice; then, at the automatic batch, at strides 12, 16 and 32 with
every subset of the three outputs, negative off and on, host and device: one variant per dimension against the same reference, and the bytes of every
variant are identical.  A reference is computed once per (case, optimize) and shared (plane_cases.ref)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import plane_cases as pc
import plane_reference as pr

pytestmark = pytest.mark.gpu

SENTINEL = -77
DESIGNED = sorted(n for n in pc.CASES if not n.startswith("scan_"))


@pytest.fixture(scope="module")
def mod():
    from rgc_slam_amd import _lib, segmentation
    return segmentation, _lib


@pytest.fixture(scope="module")
def seg(mod):
    f = mod[0].SACSegmentation(0)
    yield f
    f.setBatch(0)
    f.close()


def c_params(_lib, prm, optimize):
    p = _lib.PlaneParams()
    _lib.load().rgc_default_plane_params(C.byref(p))
    p.distance_threshold, p.probability, p.eps_angle, p.seed = prm["threshold"], prm["probability"], prm["eps_angle"], prm["seed"]
    p.max_iterations, p.optimize, p.model_type = prm["max_iterations"], optimize, prm["model"]
    p.axis[:] = prm["axis"]
    return p


def strided(cloud, stride):
    """the cloud as records of `stride` bytes: x, y, z, then columns the call must not interpret (the fourth is copied into a record's c)"""
    n = len(cloud)
    a = np.random.default_rng(stride).uniform(1, 2, (n, stride // 4)).astype(np.float32)
    a[:, :3] = cloud[:, :3]
    return a


class Dev:
    """host data in device memory of the segmenter's context"""

    def __init__(self, f, a):
        a = np.ascontiguousarray(a)
        self._f, self.host = f, a
        self.ptr = f._dev(a.nbytes)
        if a.nbytes:
            f._chk(f._L.rgc_upload(f._h, self.ptr, a.ctypes.data, a.nbytes))

    def down(self):
        out = np.empty_like(self.host)
        self._f._down(out, self.ptr)
        return out

    def free(self):
        self._f._L.rgc_device_free(self._f._h, self.ptr)


def raw(f, _lib, a, prm, optimize, samples, negative=0, want=(True, True, True), device=False, length=None):
    """rgc_plane_segment: dict of rc, n_out, coeff and the three outputs, each pre-filled with SENTINEL (None where not asked for), and the info"""
    n = len(a)
    length = pr.stream_length(prm, samples) if length is None else length
    xyzc = np.full((n, 4), SENTINEL, np.float32) if want[0] else None
    index = np.full(n, SENTINEL, np.int32) if want[1] else None
    counts = np.full(length + 3, SENTINEL, np.int32) if want[2] else None
    coeff, m, p = np.full(4, float(SENTINEL)), C.c_int(SENTINEL), c_params(_lib, prm, optimize)
    ptr = lambda x: x.ctypes.data if x is not None else None
    smp, ns = (samples.ctypes.data, len(samples)) if samples is not None else (None, 0)
    bufs = []
    try:
        if device:
            bufs = [Dev(f, a), Dev(f, xyzc) if want[0] else None, Dev(f, index) if want[1] else None]
            d = [b.ptr if b else None for b in bufs]
            rc = f._L.rgc_plane_segment(f._h, d[0], n, a.strides[0], 1, C.byref(p), smp, ns, negative, ptr(coeff), d[1], d[2], ptr(counts), C.byref(m))
            xyzc, index = (bufs[1].down() if want[0] else None), (bufs[2].down() if want[1] else None)
        else:
            rc = f._L.rgc_plane_segment(f._h, ptr(a), n, a.strides[0], 0, C.byref(p), smp, ns, negative, ptr(coeff), ptr(xyzc), ptr(index), ptr(counts), C.byref(m))
    finally:
        for b in bufs:
            if b:
                b.free()
    return dict(rc=rc, n_out=m.value, coeff=coeff, xyzc=xyzc, index=index, counts=counts, info=f.info() if rc == 0 else None)


def check(got, ref, a, prm, optimize, negative, what, measured=None):
    assert got["rc"] == 0, (what, got["rc"])
    info, n = got["info"], len(a)
    for k in ("iterations", "skipped", "positions", "best_position", "best_count"):
        assert info[k] == ref[k], (what, k, info[k], ref[k])
    assert info["n"] == n and np.array_equal(info["ransac_coeff"], ref["ransac_coeff"]), (what, info["ransac_coeff"], ref["ransac_coeff"])
    assert info["k"] == pytest.approx(ref["k"], rel=1e-12) and info["launches"] == (-(-ref["positions"] // info["batch"]) if ref["positions"] else 0), (what, info)
    if got["counts"] is not None:
        assert np.array_equal(got["counts"][:ref["positions"]], ref["counts"]) and (got["counts"][ref["positions"]:] == SENTINEL).all(), (what, got["counts"][:ref["positions"] + 3], ref["counts"])
    coeff = got["coeff"]
    refined = bool(optimize) and ref["refined"]
    assert info["refined"] == int(refined), (what, info["refined"])
    if refined:
        tol, undecided = pc.tolerances(ref, a)
        err = np.abs(coeff - ref["coeff_exact"])
        if measured is not None:
            measured.append((float((err / tol).max()), float(err.max()), ref["bound_n"]))
        assert (err <= tol).all(), (what, coeff, ref["coeff_exact"], err, tol)
        decided = ref["threshold_margin"] > undecided or np.array_equal(coeff, ref["coeff"])     # (the same fp32 model selects the same set)
    else:
        assert np.array_equal(coeff, ref["coeff"]), (what, coeff, ref["coeff"])
        decided = True
    # consistency: the rule in numpy float32 on the REPORTED coefficients selects exactly the reported points
    mask = pr.inliers_of(a, coeff.astype(np.float32), prm["threshold"])[0] if ref["found"] else np.zeros(n, bool)
    assert np.array_equal(coeff.astype(np.float32).astype(np.float64), coeff)
    written = np.flatnonzero(mask != bool(negative)).astype(np.int32)
    assert got["n_out"] == len(written) and info["n_inliers"] == int(mask.sum()), (what, got["n_out"], len(written), info["n_inliers"])
    if decided:
        assert np.array_equal(np.flatnonzero(mask), ref["inliers"]), what
    m = len(written)
    if got["index"] is not None:
        assert np.array_equal(got["index"][:m], written) and (got["index"][m:] == SENTINEL).all(), what
    if got["xyzc"] is not None:
        rows = np.zeros((m, 4), np.float32)
        rows[:, :min(a.shape[1], 4)] = a[written, :4]
        assert np.array_equal(got["xyzc"][:m], rows) and (got["xyzc"][m:] == SENTINEL).all(), what
    return decided


def same_bytes(x, y, what):
    for k in ("coeff", "xyzc", "index", "counts"):
        if x[k] is not None and y[k] is not None:
            assert x[k].tobytes() == y[k].tobytes(), (what, k)
    assert x["n_out"] == y["n_out"] and x["info"] == dict(y["info"], batch=x["info"]["batch"], launches=x["info"]["launches"]), (what, x["info"], y["info"])


def run_case(seg, _lib, name):
    c = pc.case(name)
    cloud, prm, samples = c["cloud"], c["prm"], c["samples"]
    a16 = strided(cloud, 16)
    measured, decided_all = [], True
    try:
        for optimize in (0, 1):
            ref = pc.ref(name, optimize)
            assert pc.guards(ref), name
            first = None
            for batch, device, again in itertools.product(pc.BATCHES, (False, True), (0, 1)):
                seg.setBatch(batch)
                got = raw(seg, _lib, a16, prm, optimize, samples, device=device)
                decided_all &= check(got, ref, a16, prm, optimize, 0, (name, optimize, batch, device, again), measured)
                assert got["info"]["batch"] == (batch or min(prm["max_iterations"], 64))
                first = first or got
                same_bytes(first, got, (name, optimize, batch, device, again))
            seg.setBatch(0)
            firsts, by_stride = {}, {s: strided(cloud, s) for s in (12, 16, 32)}
            for stride, want, negative, device in itertools.product((12, 16, 32), itertools.product((False, True), repeat=3), (0, 1), (False, True)):
                a = by_stride[stride]
                got = raw(seg, _lib, a, prm, optimize, samples, negative=negative, want=want, device=device)
                what = (name, optimize, stride, want, negative, device)
                check(got, ref, a, prm, optimize, negative, what)
                got["xyzc"] = None if got["xyzc"] is None else got["xyzc"][:, :3].copy()       # (the fourth column is the stride's own)
                same_bytes(firsts.setdefault(negative, got), got, what)
                if not negative:
                    same_bytes(dict(first, xyzc=None), got, what)
    finally:
        seg.setBatch(0)
    ref = pc.ref(name, 1)
    worst = max(measured, default=(0.0, 0.0, 0.0))
    print(name, "n", len(cloud), "positions", ref["positions"], "iterations", ref["iterations"], "skipped", ref["skipped"], "best", ref["best_position"], "count", ref["best_count"],
          "inliers", len(ref["inliers"]), "| refined coefficients: largest error / tolerance over the components %.3g (largest error %.3g; derived bound on a normal component %.3g, the rest of the "
          "tolerance is the float32 rounding), set compared for equality: %s" % (worst[0], worst[1], worst[2], decided_all))
    for k, v in c["expect"].items():
        assert ref[k] == v, (name, k)
    for k, v in c["minima"].items():
        assert ref[k] >= v, (name, k)
    assert decided_all or name in pc.UNDECIDED, name          # (tests/test_plane_reference.py holds that list to the reference's margins)


@pytest.mark.parametrize("name", DESIGNED)
def test_every_designed_case_equals_the_reference_in_every_variant(seg, mod, name):
    run_case(seg, mod[1], name)


@pytest.mark.parametrize("name", pc.SCANS)
def test_general_position_on_a_synthetic_scan(seg, mod, name):
    run_case(seg, mod[1], name)


@pytest.mark.parametrize("device", [False, True])
def test_a_non_finite_coordinate_is_refused_with_nothing_written(seg, mod, device):
    _lib = mod[1]
    c = pc.case("size_257")
    for at, col, bad, batch in itertools.product((0, 256), (0, 2), (np.nan, np.inf, -np.inf), (0, 1)):
        a = strided(c["cloud"], 16)
        a[at, col] = bad
        seg.setBatch(batch)
        got = raw(seg, _lib, a, c["prm"], 1, c["samples"], device=device)
        assert got["rc"] == _lib.ERR_NONFINITE, (at, col, bad, batch, got["rc"])
        assert got["n_out"] == SENTINEL and (got["coeff"] == SENTINEL).all() and (got["xyzc"] == SENTINEL).all() and (got["index"] == SENTINEL).all()
        assert (got["counts"] == SENTINEL).all()
    seg.setBatch(0)
    empty = np.ascontiguousarray(c["samples"][:0])                              # an empty stream walks the cloud all the same
    a = strided(c["cloud"], 16)
    a[256, 1] = np.nan
    assert raw(seg, _lib, a, c["prm"], 1, empty, device=device)["rc"] == _lib.ERR_NONFINITE
    got = raw(seg, _lib, strided(c["cloud"], 16), c["prm"], 1, empty, device=device)
    assert got["rc"] == 0 and got["n_out"] == 0 and not got["coeff"].any() and got["info"]["positions"] == 0 and got["info"]["best_position"] == -1


def test_an_empty_cloud_is_ok_and_too_few_points_are_refused(seg, mod):
    _lib = mod[1]
    c = pc.case("size_63")
    got = raw(seg, _lib, strided(c["cloud"], 16)[:0], c["prm"], 1, None)
    assert got["rc"] == 0 and got["n_out"] == 0 and not got["coeff"].any() and got["info"]["n"] == 0 and got["info"]["best_position"] == -1
    for n in (1, 2):
        got = raw(seg, _lib, strided(c["cloud"], 16)[:n], c["prm"], 1, None)
        assert got["rc"] == _lib.ERR_INVALID and got["n_out"] == SENTINEL and (got["coeff"] == SENTINEL).all()
    bad = np.array([[0, 1, 2], [0, 1, 63]], np.int32)
    got = raw(seg, _lib, strided(c["cloud"], 16), c["prm"], 1, bad)
    assert got["rc"] == _lib.ERR_INVALID and got["n_out"] == SENTINEL and (got["counts"] == SENTINEL).all() and (got["index"] == SENTINEL).all()


def test_range_refusals_of_a_live_context_leave_every_output_alone(seg, mod):
    """every argument the header refuses, one at a time on an otherwise good call, host and device pointers: RGC_ERR_INVALID, and coeff, n_out, the
    records, the indices and the counts keep their sentinels; rgc_plane_set_batch's range"""
    _lib = mod[1]
    L = seg._L
    c = pc.case("size_63")
    a, good = strided(c["cloud"], 16), c["prm"]
    nan, inf = float("nan"), float("inf")
    assert raw(seg, _lib, a, good, 1, c["samples"])["rc"] == 0                  # (the call the table varies is a good one)

    def refused(device=False, samples=c["samples"], cloud=a, **kw):
        got = raw(seg, _lib, cloud, dict(good, **kw), 1, samples, device=device)
        untouched = got["n_out"] == SENTINEL and (got["coeff"] == SENTINEL).all() and all((got[k] == SENTINEL).all() for k in ("xyzc", "index", "counts"))
        return got["rc"] == _lib.ERR_INVALID and untouched
    for device in (False, True):
        assert all(refused(device, threshold=v) for v in (0.0, -1.0, nan, inf, -inf, 1e-60, 1e60)), device
        assert all(refused(device, probability=v) for v in (0.0, 1.0, -0.5, 1.5, nan)) and all(refused(device, max_iterations=v) for v in (0, -5))
        assert all(refused(device, model=v) for v in (2, -1))
        assert all(refused(device, model=pr.PERPENDICULAR, eps_angle=v) for v in (-0.1, np.pi / 2 + 1e-9, nan, inf))
        assert all(refused(device, model=pr.PERPENDICULAR, axis=v) for v in ((0.0, 0.0, 0.0), (nan, 0.0, 1.0), (inf, 0.0, 0.0), (1e200, 1e200, 0.0)))
        assert all(refused(device, cloud=a[:n]) for n in (1, 2))
        for bad in ([0, 1, 63], [0, 1, -1], [0, 0, 1], [2, 1, 2], [3, 3, 3]):
            assert refused(device, samples=np.array([[0, 1, 2], bad], np.int32)), bad
    assert raw(seg, _lib, a, dict(good, model=pr.PERPENDICULAR, eps_angle=0.0, axis=(0, 0, 5)), 1, c["samples"])["rc"] == 0      # the ends of the ranges are accepted
    assert raw(seg, _lib, a, dict(good, model=pr.PERPENDICULAR, eps_angle=np.pi / 2, axis=(0, 0, 5)), 1, c["samples"])["rc"] == 0
    # what raw() cannot vary: the stride, n < 0, n_samples < 0, and each NULL
    outs = dict(coeff=np.full(4, float(SENTINEL)), xyzc=np.full((63, 4), SENTINEL, np.float32), index=np.full(63, SENTINEL, np.int32), counts=np.full(20, SENTINEL, np.int32))
    m, p, smp = C.c_int(SENTINEL), c_params(_lib, good, 1), c["samples"]

    def direct(cloud=a.ctypes.data, n=63, stride=16, prm=C.byref(p), n_samples=len(smp), coeff=outs["coeff"].ctypes.data, n_out=C.byref(m)):
        return L.rgc_plane_segment(seg._h, cloud, n, stride, 0, prm, smp.ctypes.data, n_samples, 0, coeff, outs["xyzc"].ctypes.data, outs["index"].ctypes.data,
                                   outs["counts"].ctypes.data, n_out)
    assert all(direct(stride=v) == _lib.ERR_INVALID for v in (0, 8, 14, 4100, -16)) and direct(n=-1) == _lib.ERR_INVALID and direct(n_samples=-1) == _lib.ERR_INVALID
    assert direct(cloud=None) == _lib.ERR_INVALID and direct(prm=None) == _lib.ERR_INVALID and direct(coeff=None) == _lib.ERR_INVALID and direct(n_out=None) == _lib.ERR_INVALID
    assert m.value == SENTINEL and all((v == SENTINEL).all() for v in outs.values())
    assert direct() == 0 and m.value > 0
    assert L.rgc_plane_set_batch(seg._h, -1) == _lib.ERR_INVALID and L.rgc_plane_set_batch(seg._h, _lib.PLANE_MAX_BATCH + 1) == _lib.ERR_INVALID
    assert L.rgc_plane_set_batch(seg._h, _lib.PLANE_MAX_BATCH) == 0 and raw(seg, _lib, a, good, 1, c["samples"])["info"]["batch"] == _lib.PLANE_MAX_BATCH
    assert L.rgc_plane_set_batch(seg._h, 0) == 0


def test_the_counts_of_a_cloud_that_needs_a_second_pass_of_tiles(seg, mod):
    """2 200 001 points are more 1024-point tiles than the scoring kernel's 2048 workgroups: workgroups take a second tile, keep their LDS counters across
    both and flush once.  Counts, decision and inlier indices for EQUALITY, at two batch sizes, device pointers (one upload)"""
    _lib = mod[1]
    c = pc.two_pass_case()
    a, prm = c["cloud"], c["prm"]
    assert len(a) > 2048 * 1024 and a.shape[1] == 3
    ref = pr.run(a, prm, c["samples"])
    assert pc.guards(ref) and ref["positions"] == 5 and ref["best_count"] > 500000
    d = Dev(seg, a)
    idx = Dev(seg, np.full(len(a), SENTINEL, np.int32))
    try:
        for batch in (0, 2):
            seg.setBatch(batch)
            counts, coeff, m, p = np.full(8, SENTINEL, np.int32), np.zeros(4), C.c_int(0), c_params(_lib, prm, 0)
            rc = seg._L.rgc_plane_segment(seg._h, d.ptr, len(a), 12, 1, C.byref(p), c["samples"].ctypes.data, 5, 0, coeff.ctypes.data, None, idx.ptr, counts.ctypes.data, C.byref(m))
            info = seg.info()
            assert rc == 0 and np.array_equal(counts[:5], ref["counts"]) and (counts[5:] == SENTINEL).all(), (batch, rc, counts, ref["counts"])
            assert (info["best_position"], info["best_count"], info["iterations"]) == (ref["best_position"], ref["best_count"], ref["iterations"])
            assert np.array_equal(coeff, ref["coeff"]) and m.value == len(ref["inliers"])
            got = idx.down()
            assert np.array_equal(got[:m.value], ref["inliers"]) and (got[m.value:] == SENTINEL).all(), batch
    finally:
        seg.setBatch(0)
        d.free()
        idx.free()


def test_the_python_class_and_the_ground_removed_cloud_goes_into_the_clustering(seg, mod):
    sg, _lib = mod
    from rgc_slam_amd import odometry
    c = pc.case("size_1025")
    ref = pc.ref("size_1025", 0)
    s = sg.SACSegmentation(owner=seg)
    s.setInputCloud(c["cloud"])
    s.setDistanceThreshold(c["prm"]["threshold"])
    s.setMaxIterations(c["prm"]["max_iterations"])
    s.setOptimizeCoefficients(False)
    s.setSamples(c["samples"])
    assert s.counts() is None
    inliers, coeff = s.segment(with_counts=True)
    assert np.array_equal(inliers, ref["inliers"]) and np.array_equal(coeff, ref["coeff"]) and np.array_equal(s.counts(), ref["counts"])
    assert np.array_equal(s.filter()[:, :3], c["cloud"][ref["inliers"]])
    s.setNegative(True)
    rest = s.filter()
    others = np.setdiff1d(np.arange(len(c["cloud"])), ref["inliers"])
    assert np.array_equal(rest[:, :3], c["cloud"][others]) and s.info()["n_inliers"] == len(ref["inliers"])
    ec = sg.EuclideanClusterExtraction(owner=seg)                                 # filter -> remove the ground -> cluster
    ec.setInputCloud(rest)
    ec.setClusterTolerance(0.5)
    ec.extract()
    assert len(ec.labels()) == len(others)
    # the generated stream through the class and through Preprocessor: the reference's result under the same seed
    g = dict(c["prm"], seed=5, max_iterations=20)
    want = pr.run(c["cloud"], dict(g, optimize=0), None)
    s.setSamples(None)
    s.setSeed(5)
    s.setMaxIterations(20)
    inliers, coeff = s.segment()
    assert s.counts() is None and np.array_equal(inliers, want["inliers"]) and np.array_equal(coeff, want["coeff"]) and s.info()["positions"] == want["positions"]
    pre = odometry.Preprocessor(0)
    out, idx, co = pre.planeSegmentation(c["cloud"], g["threshold"], max_iterations=20, optimize=False, seed=5)
    assert np.array_equal(idx, want["inliers"]) and np.array_equal(co, want["coeff"]) and np.array_equal(out[:, :3], c["cloud"][want["inliers"]])
